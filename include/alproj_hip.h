/*
 * alproj_hip.h -- C ABI of libalproj_hip.so: the MI355X (gfx950) implementation of the
 * camera-projection hot path of 0kam/alproj (reference v1.1.1).
 *
 * The reference is pure Python and has no FFI layer; its boundary is its public Python
 * signatures.  Each entry point below names the reference function it replaces (paths
 * relative to the reference checkout).  The Python side in alproj_amd/ binds these with
 * ctypes and keeps the reference's signatures (INTEGRATION.md shows the stub a maintainer
 * of the reference would add).
 *
 * Conventions
 *   - every function returns 0 on success, a negative ALP_E* code on failure; the message
 *     for the calling thread's last failure is alp_last_error().  Numerical problems
 *     (points behind / at the camera) are NOT errors: they surface as inf/NaN exactly like
 *     the reference (src/alproj/optimize.py:146-149).
 *   - camera parameters travel as `const double[25]` in the fixed order ALP_PARAM_ORDER
 *     (keys documented at src/alproj/project.py:157-189).
 *   - host buffers belong to the caller and are only touched during the call; device
 *     memory is owned by opaque handles released by the matching *_destroy.
 *   - one handle is used from one thread at a time (the reference is single-threaded and
 *     non-reentrant: src/alproj/optimize.py:341-351).
 *   - there is NO CPU fallback: without a usable HIP device alp_init fails with
 *     ALP_ENODEVICE and every other call fails with ALP_ENOTINIT.
 */
#ifndef ALPROJ_HIP_H
#define ALPROJ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALP_ABI_VERSION 7

/* x,y,z,fov,pan,tilt,roll,a1,a2,k1..k6,p1,p2,s1..s4,w,h,cx,cy */
#define ALP_NPARAM 25
#define ALP_PARAM_ORDER "x,y,z,fov,pan,tilt,roll,a1,a2,k1,k2,k3,k4,k5,k6,p1,p2,s1,s2,s3,s4,w,h,cx,cy"

enum alp_error {
    ALP_OK = 0,
    ALP_EINVAL = -1,     /* bad argument (NULL pointer, negative size, unknown enum) */
    ALP_ENOTINIT = -2,   /* alp_init has not succeeded in this process */
    ALP_ENODEVICE = -3,  /* no HIP device / device index out of range */
    ALP_EHIP = -4,       /* a HIP runtime call failed (message has the hipError string) */
    ALP_ERCCL = -5,      /* an RCCL call failed */
    ALP_ESTATE = -6      /* handle is missing something the call needs (e.g. observed uv) */
};

enum alp_dtype {
    ALP_F32 = 0,
    ALP_F64 = 1,
    ALP_I32 = 2,
    ALP_I64 = 3,
    ALP_U8 = 4,
    ALP_U16 = 5
};

/* Loss kinds of the population evaluation. */
enum alp_loss {
    ALP_LOSS_MEAN_DIST = 0, /* "rmse" of the reference = mean Euclidean distance,
                               src/alproj/optimize.py:176-177 */
    ALP_LOSS_HUBER = 1      /* src/alproj/optimize.py:205-212 */
};

/* Loss kinds of the least-squares normal equations (alp_normal_equations): scipy.optimize.least_squares' rho(z) of ONE
 * scalar residual r, z = (r / f_scale)^2 -- not of a point's distance: ALP_NORMAL_HUBER is not ALP_LOSS_HUBER. */
enum alp_normal_loss {
    ALP_NORMAL_LINEAR = 0,  /* rho = z */
    ALP_NORMAL_SOFT_L1 = 1, /* rho = 2 (sqrt(1 + z) - 1) */
    ALP_NORMAL_HUBER = 2,   /* rho = z for z <= 1, else 2 sqrt(z) - 1 */
    ALP_NORMAL_CAUCHY = 3   /* rho = ln(1 + z) */
};

/* ---------------------------------------------------------------- library / device --- */

int alp_abi_version(void);
const char *alp_last_error(void);

/* Select HIP device `device` for this process, create the library stream and scratch
 * buffers.  Idempotent for the same device. */
int alp_init(int device);
int alp_shutdown(void);
int alp_device_count(int *count);
/* name[len] receives the gcnArchName ("gfx950:sramecc+:xnack-"); cu_count the CU number. */
int alp_device_info(char *name, int len, int *cu_count, int64_t *hbm_bytes);
/* PCI bus id ("0000:75:00.0") of the device this process was initialised on: what tells the ranks of a
 * multi-GPU job apart in a benchmark record.  len >= 16. */
int alp_device_pci_bus_id(char *id, int len);
/* 64-bit content digest of a HOST array, computed by `threads` host threads (0 = all cores); needs no device.
 * A change of any single 8-byte word always changes the digest.  The render wrappers use it to make sure a mesh
 * kept on the device still equals the caller's arrays (the reference uploads on every call,
 * src/alproj/project.py:213-215, so an in-place edit between two calls must be seen). */
int alp_host_hash64(const void *buf, int64_t bytes, int threads, uint64_t *digest);
/* (ABI 5) out[0] = min, out[1] = max of n float64 values (n >= 1) on host threads (0: up to 8), NaN for both if any value
 * is NaN -- numpy's `a.min()`, `a.max()` in one pass: `x.min(), x.max(), y.min(), y.max()` of to_geotiff (project.py:420-423)
 * took 14-30 ms of numpy on one core for the 11.7 M rows of the 100 M-vertex frame's table, a multiple of the device's work.
 * No device needed. */
int alp_host_minmax(const double *values, int64_t n, int threads, double out[2]);
/* (ABI 5) Bring the pages of a fresh host buffer into existence before the device -> host copy that fills it:
 * madvise(MADV_HUGEPAGE) + madvise(MADV_POPULATE_WRITE) from `threads` host threads (0: 4).  A copy into pages nobody has
 * touched runs at 8-13 GB/s on the bench host (one fault per 4 KB page inside the copy), into existing pages at 56 GB/s, and
 * populating 237 MB this way takes 2.7 ms.  Advice only: where the kernel refuses, nothing changes.  No device needed. */
int alp_host_prefault(void *buf, int64_t bytes, int threads);
/* Block until everything queued on the library stream is done. */
int alp_synchronize(void);

/* HIP-event timer slots on the library stream (what bench.py brackets kernels with).
 * slot in [0, 64).  (The package's render wrappers do not use them: a frame's device time comes from
 * alp_mesh_frame_ms.) */
int alp_event_record(int slot);
int alp_event_elapsed_ms(int slot_start, int slot_stop, float *ms); /* synchronises on stop */

/* Kernel-section timer.  The entry points that mix kernels with PCIe copies (alp_residuals_batch,
 * alp_rasterize_points, alp_mesh_from_rasters, alp_render_gather, alp_render_valid_count /
 * _fetch_valid) bracket their kernel sections with HIP events on the library stream while the
 * timer is on; alp_kernel_time_ms returns (and clears) the sum over the sections since the last
 * call and their number.  For bench.py's per-kernel roofline figures; off by default. */
int alp_kernel_timing(int enable);
int alp_kernel_time_ms(float *ms, int *sections);

/* Development switches this library was compiled with, comma separated; "" for a release build
 * (see the top of csrc/alp_raster.hip: several of them render wrong images by design). */
const char *alp_build_flags(void);

/* ---------------------------------------------------------------- multi-GPU (RCCL) ---- */
/* One process per GPU.  Rank 0 calls alp_comm_unique_id and ships the 128 bytes to the
 * other ranks by any means (the Python side: a localhost socket served by its own launcher, alproj_amd/launch.py, a
 * shared file, or any callable that broadcasts 128 bytes -- alproj_amd/dist.py); every rank then
 * calls alp_comm_init.  With a communicator present, alp_eval_population sums the
 * per-candidate partial losses and the vertex counts of all ranks with ONE
 * ncclAllReduce(sum, double, P+1) per call, on the library stream.
 * A failed ncclCommInitRank returns ALP_ERCCL and alp_last_error() then holds RCCL's error string, ncclGetLastError's
 * text, this rank's world position, HIP device and PCI bus id, and the environment RCCL / ROCr read. */
#define ALP_UNIQUE_ID_BYTES 128
int alp_comm_unique_id(char id[ALP_UNIQUE_ID_BYTES]);
int alp_comm_init(const char id[ALP_UNIQUE_ID_BYTES], int rank, int world_size);
int alp_comm_destroy(void);
int alp_comm_info(int *rank, int *world_size); /* 0,1 when no communicator */
/* Broadcast `bytes` bytes of the host buffer `buf` from rank `root` to every rank (ncclBroadcast on
 * the library stream); no-op without a communicator.  The optimiser shim uses it so that every
 * rank draws the SAME population: the reference constructs its sampler without a seed
 * (src/alproj/optimize.py:410-416), which is fine for one process and silently wrong for several
 * that must all-reduce the sums of identical candidates. */
int alp_comm_bcast(void *buf, int64_t bytes, int root);
/* All-gather of host buffers of different sizes: alp_comm_allgather_counts tells every rank the byte count of every
 * rank (counts[world_size]); alp_comm_allgatherv then fills `recv` (sum of the counts) with rank 0's `send`, rank
 * 1's, ... (one ncclBroadcast per rank in one group, on the library stream).  Without a communicator: a copy.
 * LsqOptimizer (src/alproj/optimize.py:442-539) solves ONE least-squares problem over all points: with the points
 * sharded over ranks, every rank gathers the residual vector and the Jacobian rows of all shards and runs the
 * identical scipy solve on them. */
int alp_comm_allgather_counts(int64_t bytes, int64_t *counts);
int alp_comm_allgatherv(const void *send, void *recv, const int64_t *counts);

/* ---------------------------------------------------------------- point sets ---------- */
/* Device-resident set of 3-D points (GCPs or DSM vertices) -- the `obj_points` DataFrame
 * of src/alproj/optimize.py:122-141 -- plus, optionally, observed image points
 * (`img_points`, src/alproj/optimize.py:173-174).
 *
 * xyz     n x 3 row-major host array (x, y, z = easting, northing, elevation), in_dtype
 *         ALP_F32 or ALP_F64, ABSOLUTE coordinates.
 * origin  local origin subtracted (in float64) before the coordinates are stored; choose
 *         it near the camera so that float32 storage does not lose the near field.
 * precision ALP_F32: coordinates, arithmetic and outputs float32 (20 B/vertex streamed);
 *           ALP_F64: everything float64 (parity mode, 40 B/vertex).
 */
typedef struct alp_points alp_points_t;

int alp_points_create(const void *xyz, int in_dtype, int64_t n, const double origin[3],
                      int precision, alp_points_t **out);
/* The same from the three COLUMNS as they lie (x[n], y[n], z[n] contiguous): a pandas DataFrame keeps its columns as rows of a
 * block, so `obj_points[["x", "y", "z"]]` of the reference's signature (optimize.py:139-141) reaches the device without the
 * host-side interleaving `DataFrame.to_numpy()` would do (96 ms for 10 M rows on one core, measured). */
int alp_points_create_columns(const void *x, const void *y, const void *z, int in_dtype, int64_t n,
                              const double origin[3], int precision, alp_points_t **out);
int alp_points_destroy(alp_points_t *pts);
int alp_points_count(const alp_points_t *pts, int64_t *n);
/* Which form of the projection the set takes.  *row_length = W > 0: the points are a raster flattened row-major, rows of W
 * points (the last one may be shorter; recognised on the device at creation, bit for bit), and alp_project streams the
 * elevations alone (12 B/vertex in float32 instead of 20); 0: the x, y, z planes (a single row, a row longer than 65 536
 * points, anything off the grid, or ALP_NO_POINTS_GRID set).  The projected pixels are the same bits either way. */
int alp_points_layout(const alp_points_t *pts, int64_t *row_length);
/* uv: n x 2 row-major host array of observed pixel coordinates (u, v). */
int alp_points_set_observed(alp_points_t *pts, const void *uv, int in_dtype);
/* ... or the two columns u[n], v[n] as they lie (img_points[["u", "v"]], optimize.py:173-174). */
int alp_points_set_observed_columns(alp_points_t *pts, const void *u, const void *v, int in_dtype);

/* Forward projection: replaces project(), src/alproj/optimize.py:122-155 (intrinsic_mat
 * :8-44, extrinsic_mat :46-96 and _distort :98-120 fused into one kernel).
 * Results stay on the device (planar u[], v[] in the set's precision) ... */
int alp_project(alp_points_t *pts, const double params[ALP_NPARAM]);
/* ... until fetched: u_out/v_out are host arrays of n elements of out_dtype (F32/F64).  out_dtype may differ from the set's
 * precision (the reference's float64 from a float32 set): the narrower type crosses PCIe -- widened by host threads while the
 * next chunk arrives, narrowed on the device -- and no temporary of the result's size is made. */
int alp_projected_fetch(alp_points_t *pts, void *u_out, void *v_out, int out_dtype);
/* Fetch a strided sample (indices first, first+stride, ...; count elements). */
int alp_projected_fetch_strided(alp_points_t *pts, int64_t first, int64_t stride,
                                int64_t count, double *u_out, double *v_out);

/* Residual vector (observed - projected), interleaved du0,dv0,du1,dv1,... (2n doubles):
 * replaces compute_residuals(), src/alproj/optimize.py:215-237.  Needs observed uv.
 * Float64 point sets: bit for bit `observed - alp_project()`, the identity the reference has by construction
 * (:233-236) -- the kernel runs alp_project's own arithmetic.  Float32 sets: same formula, one reciprocal per
 * denominator (+-inf at a pole of the lens model, like the reference), not bit-equal to alp_project's float32. */
int alp_residuals(alp_points_t *pts, const double params[ALP_NPARAM], double *out);
/* The same for B parameter vectors in one launch (cand: B x 25 row-major; out: B x 2n doubles,
 * row b = residual vector of pose b): the D+1 evaluations of a 2-point finite-difference
 * Jacobian for LsqOptimizer, src/alproj/optimize.py:461-463, :510-528. */
int alp_residuals_batch(alp_points_t *pts, const double *cand, int64_t B, double *out);
/* Exact Jacobian of the projection at one parameter vector, for LsqOptimizer's jac="analytic" and for the standard errors
 * of fitted parameters: src/alproj/optimize.py:215-237 (the residual vector, its row order) and :442-539 (the least-squares
 * solve it feeds).  target_idx: D distinct indices into the 25 parameters, w (21) and h (22) excluded, 1 <= D <= 23.
 * out: (2n, D) row-major doubles, row 2i = d u_i / d params[target_idx[j]], row 2i + 1 = d v_i / ...; of_residuals != 0
 * gives the Jacobian of observed - projected instead (its negation; no observed uv needed).  Float64 arithmetic on either
 * set; the derivative of exactly the model alp_project evaluates (the reference's distortion, its quirks included).
 * ALP_EINVAL for NULL, a bad D, a bad or repeated target.  n = 0: nothing happens. */
int alp_jacobian(alp_points_t *pts, const double params[ALP_NPARAM], const int32_t *target_idx, int D, int of_residuals,
                 double *out);
/* The normal equations of the least-squares problem at one parameter vector, formed on the device: what a Gauss-Newton /
 * Levenberg-Marquardt step and the covariance s^2 (J^T J)^-1 need of the residual vector of src/alproj/optimize.py:215-237
 * and of the solve of :442-539, without the (2n, D) Jacobian ever leaving the registers.  J = the Jacobian of the residual
 * vector observed - projected (alp_jacobian with of_residuals), r = that vector (a float64 set: alp_residuals' values bit
 * for bit); float64 arithmetic on either set.  loss (enum alp_normal_loss) and f_scale have scipy's meaning: with
 * z = (r_i / f_scale)^2, row i of J is scaled by s_i = sqrt(max(rho'(z) + 2 z rho''(z), 1e-10)) and r_i by rho'(z) / s_i
 * (linear: s = 1).  Targets as for alp_jacobian.  out, D (D + 1) / 2 + D + 2 doubles:
 *   the upper triangle of J^T J, row-major | J^T r (D values) | sum of rho(z) (cost = f_scale^2 / 2 times it) | point count.
 * With a communicator, every value is the sum over the ranks (one all-reduce of at most 301 doubles).  No atomics: the
 * order of every addition is set by the launch shape, so the same call gives the same bits.  Non-finite values propagate
 * into the sums they touch.  n = 0 gives zeros.  Needs observed uv (else the error alp_residuals gives).
 * ALP_EINVAL for NULL, a bad D, a bad or repeated target, an unknown loss, f_scale <= 0 or not finite. */
int alp_normal_equations(alp_points_t *pts, const double params[ALP_NPARAM], const int32_t *target_idx, int D, int loss,
                         double f_scale, double *out);
/* alp_normal_equations for B parameter vectors in one launch: what a multi-start Levenberg-Marquardt needs per round -- the
 * sums of the residual vector of src/alproj/optimize.py:215-237 at the trial points of B independent solves of :442-539 (K
 * starts polished side by side, as the K candidate optima of the multi-start form of the CMA-ES loop of :359-439 leave them).
 * params: B x ALP_NPARAM row-major, 1 <= B <= 1024; targets, loss and f_scale are shared by the rows.  out: B rows of
 * D (D + 1) / 2 + D + 2 doubles, row b in alp_normal_equations' layout for params row b (the point count is repeated in every
 * row).  One workgroup per (stripe of points, pose) pair; a pose's stripes are added in stripe order, no atomics: a row does
 * not depend on the other rows of the call, and the same call gives the same bits.  alp_normal_equations is the B = 1 case
 * of this launch: a row has the bits of the single call wherever B poses get the stripes one pose gets -- the device's
 * workgroups (6 per CU, at most 2048) are shared out among the poses, ceil(that / B) stripes each, at most one per group of
 * 256 points; so always up to 256 points, and for any n while that share is at least the number of groups.  Elsewhere the
 * stripes are cut differently and the two agree to the reassociation of the sums.  With a communicator: one all-reduce of B (D (D + 1) / 2 + D + 2) doubles.  n = 0 gives B rows
 * of zeros.  Errors as for alp_normal_equations (same codes; ALP_ESTATE without observed uv), and ALP_EINVAL for B < 1 or
 * B > 1024. */
int alp_normal_equations_batch(alp_points_t *pts, const double *params, int64_t B, const int32_t *target_idx, int D, int loss,
                               double f_scale, double *out);
/* alp_normal_equations_batch with every pose under a weight row of its own: pose b is evaluated under row row_of_pose[b]
 * (0 .. R-1, repeats allowed, B need not be R) of the table of alp_points_set_weight_table instead of under the weight plane --
 * the K folds of a cross-validation or the resamples of a bootstrap of the solve of src/alproj/optimize.py:442-539 in the
 * launch the K starts take.  out as for alp_normal_equations_batch, except that the count slot of row b carries the sum of
 * ITS weight row (over the ranks, through the same all-reduce).  Grid, stripes and the order of every addition are
 * alp_normal_equations_batch's for the same B: row b has, bit for bit, the values alp_points_set_weights(row row_of_pose[b])
 * followed by alp_normal_equations_batch gives, and depends on no other row of the call; a row whose weights are all 0 gives
 * exact zeros and count 0.  Errors as for alp_normal_equations_batch, ALP_ESTATE when no table is set, ALP_EINVAL for a row
 * index outside the table (checked on the host before the launch). */
int alp_normal_equations_batch_rows(alp_points_t *pts, const double *params, int64_t B, const int32_t *row_of_pose,
                                    const int32_t *target_idx, int D, int loss, double f_scale, double *out);
/* Residuals with the pose chosen per POINT, in one launch: point i is evaluated under params row assign[i] (cand: B x 25
 * row-major, 1 <= B <= 4096; assign: n values in -1 .. B-1).  out: 2n doubles in alp_residuals' order (the residual vector of
 * src/alproj/optimize.py:215-237), a NaN pair where assign[i] < 0.  With assign = the fold of every point and cand = the optima
 * fitted without that fold, these are the held-out residuals of a cross-validation.  Float64 arithmetic on either set; on a
 * float64 set the pair of point i has the bits of row assign[i] of alp_residuals_batch.  Needs observed uv (ALP_ESTATE);
 * ALP_EINVAL for NULL, B out of range or an assign[i] >= B (checked on the host before the launch).  n = 0: nothing happens. */
int alp_residuals_assigned(alp_points_t *pts, const double *cand, int64_t B, const int32_t *assign, double *out);

/* Population-wide reprojection error: replaces the inner loop of CMAOptimizer.optimize,
 * src/alproj/optimize.py:420-423, i.e. P calls of _proj_error (:347-356) = project +
 * rmse (:157-178) or huber_loss (:181-212).
 *
 * cand      P x 25 row-major candidate parameter vectors (already de-normalised).
 * loss_out  P doubles: mean over ALL vertices (of all ranks when a communicator exists).
 * argmin_out index of the smallest loss, first index on ties, NaN never wins unless all
 *           are NaN (then 0) -- the contract of solutions[0] after CMA.tell's stable sort,
 *           src/alproj/optimize.py:424-427.
 * Float32 point sets: when other losses lie within 5e-5 (relative) of the smallest, up to 16
 * of those candidates are evaluated again in float64 arithmetic on the stored points before
 * the index is returned (the north star's "argmin bit-exact"); loss_out then holds the
 * float64 re-evaluations for THOSE candidates and the float32-path losses for all others.
 * Poles of the rational lens model (src/alproj/optimize.py:112-116: a vertex for which EXACTLY one of
 * 1 + k4 r2 + k5 r4 + k6 r6 and 1 + a2 + k4 r2 + ... is zero): the reference's coordinate on that axis is +-inf, the
 * other finite, the candidate's loss +inf.  The kernel shares one reciprocal between the two denominators, which
 * turns the finite coordinate into NaN.  FLOAT64 point sets (the parity mode) mend it: a wave whose sum for a candidate
 * comes out infinite or NaN walks its share of the points again for that candidate with a reciprocal per denominator,
 * so the loss is +inf as in the reference (NaN only where the reference is NaN too).  FLOAT32 point sets keep the NaN:
 * the loss of such a candidate is NaN where the reference has +inf -- it ranks last either way (argmin_out skips NaN,
 * CMA.tell sorts NaN as +inf); a wild float32 population has overflow NaNs in a third of its candidates anyway, which no
 * second walk can mend.  tests/test_gpu_points.py constructs the case in both modes.
 * Lens-free populations (ALP_POP_LENS_FREE, below) take the second walk in either precision: it restores the NaN the
 * reference's k * inf produces at a vertex at the camera.
 * Mended losses (float32 point sets, alp_points_set_mend; off by default): with mend on, every candidate whose float32 sum
 * comes out infinite or NaN is evaluated again on the device -- no host round trip, in the device loop as well -- in float64
 * ARITHMETIC ON THE STORED FLOAT32 POINTS and observations, second walk included, and loss_out holds that value for it;
 * every other candidate keeps its float32 loss bit for bit.  A wild float32 population is then finite wherever float64
 * arithmetic is: a vertex next to a candidate's camera plane has a squared pixel distance above FLT_MAX in float32 (inf -
 * inf = NaN follows), which float64 holds with room to spare.  A mended loss is exact for the stored inputs (1e-7 relative
 * and better against float64 arithmetic on the same rounded points); it is NOT the reference's loss to 1e-5, because the
 * reference reads the unrounded points: float64 arithmetic on the fixture's points and observations rounded as a float32 set
 * stores them differs from the fixture's own losses by 4.2e-4 relative at a candidate whose smallest lens denominator is
 * 3.3e-4, and by 1.5e-4 at one with a depth ratio of 5e-5.  That floor is the float32 input's, and no re-evaluation on the
 * stored planes lowers it.  A candidate whose re-evaluation is itself not finite keeps that value, which is the reference's
 * own: +inf at an exact pole (not the NaN above), NaN at a vertex at the camera.
 * argmin_out == NULL: losses only, no confirmation pass (the reference uses the argmin of the LAST
 * generation only, src/alproj/optimize.py:427; every earlier generation needs the losses for
 * CMA.tell and nothing else).
 * Reproducibility (argmin_out == NULL): the losses are bit-identical for the same point set, P, kernel variant
 * (alp_eval_population_info) and launch grid, and a candidate's loss does not depend on its slot in cand or on the other
 * candidates.  Across launch grids (and so across point counts and tile counts) they agree to the last bits only: ~3e-8
 * relative in float32, whose grid decides which rows are summed in which group, ~1e-15 in float64.
 */
int alp_eval_population(alp_points_t *pts, const double *cand, int64_t P, int loss_kind,
                        double f_scale, double *loss_out, int64_t *argmin_out);
/* Same, but only enqueues the work on the library stream (H2D of the candidate records,
 * kernels, all-reduce, D2H into an internal pinned buffer).  alp_eval_population_wait
 * synchronises and delivers the results of the last enqueue. */
int alp_eval_population_enqueue(alp_points_t *pts, const double *cand, int64_t P,
                                int loss_kind, double f_scale);
int alp_eval_population_wait(alp_points_t *pts, double *loss_out, int64_t *argmin_out);
/* Device time of the last completed population evaluation of this handle, from HIP events on the
 * library stream: kernel_ms = the evaluation and reduction kernels, allreduce_ms = the
 * ncclAllReduce(sum, double, P+1) behind them (about 0 without a communicator); when the evaluation ran the mend pass
 * (alp_points_set_mend), kernel_ms includes it.  What bench.py
 * reports as the collective's share of a CMA-ES generation (src/alproj/optimize.py:418-424 has no
 * counterpart: the reference is one process). */
int alp_eval_population_timing(alp_points_t *pts, float *kernel_ms, float *allreduce_ms);
/* (ABI 7) Which kernel variant the last population evaluation of this handle was given, and its launch shape:
 * info[0] = ALP_POP_GENERAL, ALP_POP_SHARED_POSE (every candidate has the same position / angles / fov: the reference's second
 * phase, example.py:75-78 -- the transform is hoisted out of the candidate loop) or ALP_POP_LENS_FREE (no candidate has a lens
 * coefficient other than a1, a2: the reference's first phase, example.py:51-54 -- the lens is folded into the pose rows on
 * the host and optimize.py:112-118 costs no arithmetic per point); info[1] = stripes of points, info[2] = columns of
 * candidate tiles of the launch grid.  The losses of one candidate agree between the variants to the tolerances of the
 * precision mode (float64: 1e-12 relative; float32: 2e-6), not bit for bit. */
enum alp_pop_variant { ALP_POP_GENERAL = 0, ALP_POP_SHARED_POSE = 1, ALP_POP_LENS_FREE = 2 };
int alp_eval_population_info(alp_points_t *pts, int64_t info[3]);
/* The mend pass of a float32 point set (see alp_eval_population): a per-handle setting, off at creation.  ALP_ESTATE while an
 * evaluation is enqueued or a device loop on the set has generations pending.  A float64 set accepts the call and never runs
 * the pass (its second walk gives the reference's values already).  Enabling it (from off) clears the running total below.
 * With a communicator the pass adds one all-reduce of P doubles per evaluation; every rank must use the same setting.
 * alp_eval_population_timing counts the pass (select, float64 evaluation, reduction, its all-reduce, scatter) as kernel time. */
int alp_points_set_mend(alp_points_t *pts, int enable);
/* info[0] = candidates the mend pass re-evaluated in the last completed population evaluation (a device loop: in its last
 * generation; 0 when that evaluation ran no pass), info[1] = their total since mend was enabled, info[2] = stripes and
 * info[3] = candidate-tile columns of the pass's launch grid (planned for all P candidates; 0, 0 without a pass).
 * ALP_ESTATE before any evaluation and while one is pending. */
int alp_eval_population_mended(alp_points_t *pts, int64_t info[4]);

/* Per-point frequency weights.  w: n host values of in_dtype (ALP_F32 or ALP_F64), finite and >= 0, one per point; NULL clears
 * them.  They are stored in the set's element type -- a float32 set ROUNDS them to float32 -- as one more plane (4 B/point in
 * float32, 8 B/point in float64) that the population kernels and the normal-equation kernels read beside the observed pixels.
 * With W = sum w_i over all ranks:
 *   alp_eval_population*, the CMA-ES device loop: mean distance = sum w_i d_i / W, Huber = sum w_i huber(d_i) / W -- for
 *     integer weights the losses of the set in which point i appears w_i times.  The float64 confirmation of near-tied float32
 *     losses and the mend pass use the same weights.
 *   alp_normal_equations*, the least-squares device loop: both residual rows of point i count w_i times (row scalings times
 *     sqrt(w_i), cost += w_i rho): J^T J, J^T r and the cost of that set, for all four losses.
 *   The count slot of every one of these results (the last value of alp_normal_equations' `out`, of each row of the batch)
 *     carries W instead of n.
 * A point of weight 0 is ABSENT: its term is selected away even when its distance is NaN or infinite (a vertex at the camera or
 * on the camera plane does not poison the sums).  A positive weight keeps the NaN / inf behaviour of an unweighted point.  Unit
 * weights give the bits of the set without weights.  alp_project, alp_residuals*, alp_jacobian and alp_loss_uv* ignore the
 * weights, and a set without weights runs exactly the kernels it ran before this call existed.
 * ALP_EINVAL for a negative, NaN or infinite weight (checked on the host before anything is uploaded: the previous weights
 * stay in force); ALP_ESTATE while an evaluation is enqueued or a device loop on the set is pending.  With a communicator
 * every rank sets the weights of its own shard; a shard whose weights are all 0 is fine as long as W > 0. */
int alp_points_set_weights(alp_points_t *pts, const void *w, int in_dtype);
/* *W = the float64 sum of this rank's stored (rounded) weights, added in index order; n when no weights are set. */
int alp_points_weight_sum(const alp_points_t *pts, double *W);

/* A TABLE of weights: R rows of n weights each, row-major (w: R x n host values of in_dtype), for the calls that evaluate
 * every pose under a row of its own -- alp_normal_equations_batch_rows and the device loop of alp_lm_create_rows.  Values,
 * storage (the set's element type: a float32 set rounds) and the meaning of a weight are alp_points_set_weights'; so are the
 * rules: everything is validated on the host before anything changes (ALP_EINVAL for a negative, NaN or infinite weight or
 * one that does not fit the element type: the previous table stays in force), w = NULL drops the table, ALP_ESTATE while an
 * evaluation is enqueued or a device loop on the set is pending.  1 <= R <= 1024, and the stored table holds at most
 * ALP_WEIGHT_TABLE_MAX_BYTES (R n element sizes; ALP_EINVAL above) -- a guard, not a tuned number.  The table and the
 * plane of alp_points_set_weights are independent: a call that names table rows ignores the plane, every other call ignores the
 * table and runs the kernels it ran before.  The sum of every stored row is formed on the device when the table is set, in
 * float64, without atomics and in an order that depends on n alone, and kept beside the table: the count slots come from
 * there.  With a communicator every rank sets the columns of its own shard. */
#define ALP_WEIGHT_TABLE_MAX_BYTES ((int64_t)1 << 30)
int alp_points_set_weight_table(alp_points_t *pts, const void *w, int R, int in_dtype);
/* out[0 .. R) = this rank's row sums as the device formed them; ALP_ESTATE when no table is set. */
int alp_points_weight_table_sums(alp_points_t *pts, double *out);

/* The candidate sampler of the CMA-ES loop on the device: replaces the `population_size` calls of
 * `optimizer.ask()` per generation, src/alproj/optimize.py:420-421 (third-party cmaes==0.12.0,
 * requirements.txt:14; bounds handling documented at optimize.py:381-384).  Candidate c of generation g:
 * x = mean + sigma * BD z with z ~ N(0, I_D) (BD = B diag(D) of the covariance C = B D^2 B^T, D x D
 * row-major); a draw outside [lower, upper] is re-drawn, the first feasible one of n_max_resampling tries
 * wins, otherwise draw number n_max_resampling is clipped to the box.  lower = upper = NULL: no box.
 * Counter-based (Philox4x32-10 keyed by seed; counter = try, candidate, generation): the same numbers on
 * every rank.  x_out: P x D row-major host array; tries_out (optional, P ints): index of the draw used
 * (n_max_resampling = clipped).  D <= 32. */
int alp_cma_sample(const double *mean, double sigma, const double *BD, const double *lower, const double *upper,
                   int D, int64_t P, int n_max_resampling, uint64_t seed, uint64_t generation, double *x_out,
                   int32_t *tries_out);

/* ---------------------------------------------------------------- device loop of the CMA-ES generation --- */
/* Generations of CMAOptimizer.optimize (src/alproj/optimize.py:410-427: ask, evaluate, tell) enqueued on the library stream
 * with the optimiser's state on the device: no copy to the host and no synchronisation between generations
 * (CMAOptimizer.optimize(..., device_loop=True); the host loop stays the default).  One generation is three launches:
 * the draw of alp_cma_sample from the device state (the same bits for the same seed, generation, mean, sigma and BD) with
 * the de-normalisation x * (upper - lower) + lower, the candidate matrix and the fold of every pose; the population
 * evaluation of alp_eval_population (+ the all-reduce of its sums when a communicator exists); and the tell of cma.py
 * (losses = sums / n_total, stable ascending order with NaN as +inf, mean / p_sigma / sigma / pc / C updates in numpy's
 * order, then the eigendecomposition of C for the next generation), one workgroup in float64.
 * The handle uses the population scratch of `pts`: while generations are enqueued, alp_eval_population_enqueue on `pts`
 * returns ALP_ESTATE, and so does every call on the handle but alp_cma_wait / alp_cma_destroy.  A handle whose point set
 * has been destroyed returns ALP_ESTATE from alp_cma_run. */
typedef struct alp_cma alp_cma_t;
/* hyper[ALP_CMA_NHYPER] = {mu, mu_eff, c1, cmu, cc, c_sigma, d_sigma, chi_n, cm, sum(weights)} and weights[P]: the constants of
 * the host cma.CMA object (alproj_amd/cma.py), passed as it computed them. */
#define ALP_CMA_NHYPER 10
/* tmpl: the 25 ABI parameters of params_init; target_idx[D]: the ABI index of every target (not w, h); lower / upper[D]: the
 * bounds of the targets (optimize.py bounds_to_array); P <= 4096, D <= 32.  The state starts as a fresh CMA's (mean 0.5,
 * sigma 1, C = I); alp_cma_set_state sets it.  The kernel variant of the evaluation is chosen here, by the rules of
 * alp_eval_population: lens-free (no target in k1..s4, the template's k1..s4 all 0; not under ALP_POP_NO_LENS_FREE), else
 * shared pose (every target in a1..s4, P > 1), else general.  The handle keeps `pts`; destroy it before the point set. */
int alp_cma_create(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                   const double *upper, int64_t P, const double *weights, const double hyper[ALP_CMA_NHYPER], int n_max_resampling,
                   uint64_t seed, alp_cma_t **out);
int alp_cma_destroy(alp_cma_t *h);
/* mean[D], sigma, C[D x D] row-major, p_sigma[D], pc[D], generation (cma.py get_state / set_state); set_state then runs the
 * eigendecomposition of C (cma.py _eigen: C is symmetrised and rewritten as B diag(d^2) B^T).  get_state: every output may be
 * NULL; B[D x D] (eigenvectors as columns) and Dvec[D] are those the next draw uses (BD = B diag(Dvec)). */
int alp_cma_set_state(alp_cma_t *h, const double *mean, double sigma, const double *C, const double *p_sigma, const double *pc,
                      int64_t generation);
int alp_cma_get_state(alp_cma_t *h, double *mean, double *sigma, double *C, double *p_sigma, double *pc, int64_t *generation, double *B,
                      double *Dvec);
/* Enqueue `generations` generations (enqueue only; alp_cma_wait synchronises).  A second run before the wait: ALP_ESTATE. */
int alp_cma_run(alp_cma_t *h, int64_t generations, int loss_kind, double f_scale);
int alp_cma_wait(alp_cma_t *h);
/* One tell on given candidates X[P x D] (normalised) and losses[P], then the eigendecomposition; order_out (optional, P
 * ints): the order the tell sorted by (cma.py tell_population's return value).  For tests. */
int alp_cma_tell_host(alp_cma_t *h, const double *X, const double *losses, int32_t *order_out);
/* The last device generation: X[P x D] (normalised draws), cand[P x 25] (the candidate matrix), losses[P]; any may be NULL.
 * For tests. */
int alp_cma_fetch_last(alp_cma_t *h, double *X, double *cand, double *losses);
/* Multi-start (CMAOptimizer.optimize(..., starts=K)): K independent states that share D, P, the targets, bounds, weights and
 * hyperparameters; start k draws with seeds[k].  One generation is still three launches: the draw of K * P candidates (row
 * k * P + i is draw i of start k, the bits of alp_cma_sample(..., seeds[k], g) from start k's state), one evaluation of K * P
 * candidates (+ one all-reduce of K * P + 1 sums), and a tell of K workgroups, one per start.  1 <= K <= 1024, K * P <= 65536;
 * alp_cma_create is the case K = 1.  On a K-start handle alp_cma_tell_host and alp_cma_fetch_last take and return K * P rows
 * in start order (the order is per start: indices 0 .. P-1 within each start's rows); alp_cma_set_state / alp_cma_get_state
 * are start 0.  The evaluation scratch of `pts` grows to K * P candidates; for K > 1 its partial sums stay within 128 MB. */
int alp_cma_create_starts(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                          const double *upper, int64_t P, int K, const double *weights, const double hyper[ALP_CMA_NHYPER],
                          int n_max_resampling, const uint64_t *seeds, alp_cma_t **out);
/* alp_cma_set_state / alp_cma_get_state of start k (0 <= k < K, else ALP_EINVAL). */
int alp_cma_set_state_at(alp_cma_t *h, int k, const double *mean, double sigma, const double *C, const double *p_sigma, const double *pc,
                         int64_t generation);
int alp_cma_get_state_at(alp_cma_t *h, int k, double *mean, double *sigma, double *C, double *p_sigma, double *pc, int64_t *generation,
                         double *B, double *Dvec);

/* ---------------------------------------------------------------- device loop of the least-squares iteration --- */
/* K bounded Levenberg-Marquardt runs on the normal equations (LsqOptimizer.optimize(method="normal", starts=K,
 * device_loop=True): the solve of src/alproj/optimize.py:442-539 on the sums of the residual vector of :215-237) with their
 * state on the device: rounds are enqueued on the library stream with no copy to the host and no synchronisation between them.
 * The iteration is alproj_amd/optimize.py: _normal_lm_steps, statement by statement (csrc/host/alp_lm.h).  One round:
 *   the evaluation   alp_normal_equations_batch's kernel over the starts that still run, on the grid of all K starts (a start's
 *                    stripes, and so the order of its additions, do not depend on which other starts have stopped), its
 *                    reduction, and -- with a communicator -- one all-reduce of K (D (D + 1) / 2 + D + 2) doubles
 *   the step         one workgroup per start: consume the sums at the trial point (accept / reject, gain ratio, damping
 *                    update, ftol / xtol), then produce the next trial point (gtol / max_nfev, free set, damped Cholesky solve,
 *                    clip, predicted reduction) or stop; for a start that goes on, the 25-parameter row and its plan
 *                    (the fold of the pose and its derivative for every target, csrc/host/alp_jacplan.h) are built there too
 *   the selection    the list of the starts that still run, ascending
 * No atomics anywhere: the same handle history gives the same bits.  A device run's trajectory is NOT the host run's: the
 * plan's sines and cosines and the solve round differently from libm and LAPACK, and near convergence `cost_new < cost` is
 * decided at rounding level, so evaluation counts and the status among 2 / 3 / 4 may differ. */
typedef struct alp_lm alp_lm_t;
/* The status alp_lm_get reports for a start that has not stopped (no stop uses it; the stops are normal_lm's: -1, 0 .. 4). */
#define ALP_LM_RUNNING (-2)
/* tmpl: the 25 ABI parameters of params_init; target_idx[D]: the targets, by alp_jacobian's rule (1 <= D <= 23, distinct, not w
 * or h); lower / upper[D]: the box (either may be infinite); X0[K x D]: the starts (clipped into the box), 1 <= K <= 1024;
 * loss / f_scale as for alp_normal_equations; ftol, xtol, gtol and max_nfev (>= 1, per start) with scipy's meaning.  Prepares the
 * first trial points (X0 clipped), their plans and the list.  Needs observed uv (ALP_ESTATE).  The handle keeps `pts`; destroy it
 * before the point set (a handle whose point set is gone returns ALP_ESTATE from alp_lm_run). */
int alp_lm_create(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                  const double *upper, const double *X0, int K, int loss, double f_scale, double ftol, double xtol, double gtol,
                  int64_t max_nfev, alp_lm_t **out);
/* alp_lm_create with start k evaluated under row k of the table of alp_points_set_weight_table (which must have exactly K rows:
 * ALP_EINVAL otherwise, ALP_ESTATE without a table) instead of under the weight plane: K fits of K resamples in one loop.  The
 * evaluation is alp_normal_equations_batch_rows' for row_of_pose = 0 .. K-1; everything else is alp_lm_create's.  Replacing the
 * table by one of another height makes alp_lm_run return ALP_ESTATE. */
int alp_lm_create_rows(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                       const double *upper, const double *X0, int K, int loss, double f_scale, double ftol, double xtol, double gtol,
                       int64_t max_nfev, alp_lm_t **out);
int alp_lm_destroy(alp_lm_t *h);
/* Enqueue `rounds` rounds (enqueue only; alp_lm_wait synchronises).  A second run before the wait: ALP_ESTATE.  Rounds after
 * the last start has stopped do nothing. */
int alp_lm_run(alp_lm_t *h, int64_t rounds);
/* Synchronise; *pending = the number of starts that have not stopped (8 bytes cross PCIe). */
int alp_lm_wait(alp_lm_t *h, int64_t *pending);
/* The K records; any output may be NULL.  x[K x D]: the current point (the result once stopped), cost, grad_norm (the infinity
 * norm of g over the free variables; NaN with status -1), iterations (accepted steps), evaluations, status (ALP_LM_RUNNING for
 * a start that has not stopped), trial[K x D]: the pending trial point, mu / nu: the damping. */
int alp_lm_get(alp_lm_t *h, double *x, double *cost, double *grad_norm, int64_t *iterations, int64_t *evaluations, int32_t *status,
               double *trial, double *mu, double *nu);
/* One round whose evaluation is replaced by the given sums: K rows in alp_normal_equations_batch's layout
 * (D (D + 1) / 2 + D + 2 doubles; the rows of stopped starts are ignored).  Step and selection run, then it synchronises.
 * For tests. */
int alp_lm_step_host(alp_lm_t *h, const double *sums);

/* Loss of two host arrays of pixel coordinates (n x 2 row-major doubles each): replaces the
 * stand-alone rmse(), src/alproj/optimize.py:157-178 (loss_kind ALP_LOSS_MEAN_DIST) and
 * huber_loss(), :181-212 (ALP_LOSS_HUBER).  Float64 arithmetic on the device. */
int alp_loss_uv(const double *observed, const double *projected, int64_t n, int loss_kind,
                double f_scale, double *loss_out);
/* The same with either array given as its two COLUMNS as they lie in a table (obs_u[n], obs_v[n] / prj_u[n], prj_v[n]); an
 * array whose second pointer is NULL is taken as interleaved n x 2 like alp_loss_uv's.  `projected` is what project()
 * returned -- a DataFrame whose u, v are two separate runs -- so the reference's call rmse(img_points, projected) needs no
 * host-side interleaving (90 -> ~8 ms at 10 M rows).  Same sum order as alp_loss_uv: the same bits. */
int alp_loss_uv_columns(const double *obs_u, const double *obs_v, const double *prj_u, const double *prj_v, int64_t n,
                        int loss_kind, double f_scale, double *loss_out);

/* ---------------------------------------------------------------- mesh render --------- */
/* Device-resident triangle mesh: the vbo/cbo/ibo of src/alproj/project.py:213-215.
 *
 * vert   n_vert x 3, X, Z(up), Y order, relative to `offsets` (src/alproj/surface.py:189-190,
 *        :211); vert_dtype ALP_F32, or ALP_F64 -- what get_colored_surface returns: the cast of
 *        src/alproj/project.py:213 (astype("f4"), round to nearest even) then happens on the
 *        device during the chunked upload, no float32 copy is made on the host.
 * value  n_vert x 3 per-vertex values (colours, or the vertices themselves for reverse_proj,
 *        src/alproj/project.py:360), value_dtype ALP_F32 or ALP_F64 (cast of :214 likewise);
 *        NULL means value == vert.
 * ind    n_tri x 3 indices (ind_dtype ALP_I32 or ALP_I64), or NULL for the implicit
 *        regular grid of src/alproj/surface.py:194-201 with grid_h x grid_w vertices
 *        (n_vert == grid_h * grid_w; vertex id = row * grid_w + col).
 *        An index array that IS that grid, or that grid with the triangles of nodata
 *        vertices removed (src/alproj/surface.py:203-205, order kept), is recognised and
 *        rendered by the grid kernels (same result, no 12 B/triangle index reads); the full
 *        grid is recognised by host threads while the vertices are uploaded (or, without
 *        threads to spare, while it streams through the staging buffer) and is never stored;
 *        triangle ids reported by alp_render_fetch_visibility stay positions in `ind`.
 *        Indices outside [0, n_vert) are rejected (ALP_EINVAL; checked on the device).
 * (ABI 3: vert_dtype / value_dtype added; ABI 2 took float32 pointers only.)
 */
typedef struct alp_mesh alp_mesh_t;

int alp_mesh_create(const void *vert, int vert_dtype, const void *value, int value_dtype,
                    int64_t n_vert, const void *ind, int ind_dtype, int64_t n_tri,
                    int64_t grid_h, int64_t grid_w, alp_mesh_t **out);
int alp_mesh_destroy(alp_mesh_t *mesh);
/* How the mesh is held: info[0] = 1 when it is rendered as the implicit regular grid (given as
 * one, or an index array recognised as one -- possibly with a derived vertex mask), 0 when
 * through its index array; info[1], info[2] = grid rows, columns (0 for index meshes);
 * info[3] = number of triangles the kernels enumerate. */
int alp_mesh_info(alp_mesh_t *mesh, int64_t info[4]);

/* Replace (or, with NULL, drop) the stored per-vertex values of a resident mesh: sim_image's
 * colours for a mesh that reverse_proj created without any, src/alproj/project.py:214.  The
 * vertices, the index array and the visibility cache (below) are untouched. */
int alp_mesh_set_value(alp_mesh_t *mesh, const void *value, int value_dtype);

/* What the following renders interpolate: the stored per-vertex values (sim_image,
 * src/alproj/project.py:321) or the vertices themselves (reverse_proj, project.py:360) -- one
 * resident mesh serves both calls of the reference's pipeline (example.py:33-36). */
enum alp_value_source { ALP_VALUE_STORED = 0, ALP_VALUE_VERTICES = 1 };
int alp_mesh_set_value_source(alp_mesh_t *mesh, int source);

/* Per-vertex nodata mask (n_vert bytes, 0 = nodata; NULL removes the mask): triangles touching
 * a masked vertex are not drawn -- what get_colored_surface does by filtering its index array,
 * src/alproj/surface.py:203-205.  Triangle ids stay those of the unfiltered mesh. */
int alp_mesh_set_valid(alp_mesh_t *mesh, const uint8_t *valid);

/* Mesh construction of get_colored_surface() after its raster I/O, src/alproj/surface.py:173-212,
 * on the device: implicit-grid mesh with colours and nodata mask from
 *   dsm      rows x cols elevations (ALP_F32 or ALP_F64), nodata already filled (:171);
 *            clamped to [0, z_max] (:175-176, z_max = the `dsm_max_height` of :169)
 *   transform  the six affine coefficients a, b, c, d, e, f of the merged rasters:
 *            x = col * a + c, y = row * e + f (:179-180)
 *   aerial   3 x rows x cols band-planar colours (ALP_U8, ALP_U16 or ALP_F32), divided by
 *            color_div (0 = leave as they are) and clipped to [0, 1] (_normalize_aerial, :26-66;
 *            the caller picks the divisor from the source dtype / color_max)
 *   nodata   rows x cols bytes, nonzero = DSM nodata (:110-117), or NULL
 * Vertices are float32 (x, z, y) minus offsets_out = their float64 minimum (:211-212), vertex id
 * = row * cols + col, triangles (a, a+cols, a+cols+1), (a, a+cols+1, a+1) (:194-201). */
int alp_mesh_from_rasters(const void *dsm, int dsm_dtype, int64_t rows, int64_t cols,
                          const double transform[6], double z_max, const void *aerial,
                          int aerial_dtype, double color_div, const uint8_t *nodata,
                          double offsets_out[3], alp_mesh_t **out);

/* Copy the resident mesh back (any pointer may be NULL): vert, value n_vert x 3 float32, valid
 * n_vert bytes.  For inspection and parity tests. */
int alp_mesh_fetch(alp_mesh_t *mesh, float *vert, float *value, uint8_t *valid);

/* Depth-buffered render + lens-distortion remap: replaces persp_proj(),
 * src/alproj/project.py:145-294 (OpenGL draw :210-290, distort :111-143).
 *
 * params        camera parameters, ABSOLUTE camera position.
 * offsets       the 3 offsets (X,Z,Y order) subtracted from the camera position
 *               (src/alproj/project.py:204-207), or NULL.
 * min_distance  <= 0 disables the near-field mask (src/alproj/project.py:247, :264).
 * out           h x w x 3 float32 host image, row 0 = top (after the flipud of :281).
 */
int alp_render(alp_mesh_t *mesh, const double params[ALP_NPARAM], const double *offsets,
               double min_distance, float *out);
/* Same but leaves the image on the device (for timing); fetch with alp_render_fetch.
 *
 * Visibility cache: the reference renders the same mesh twice at one pose -- sim_image, then
 * reverse_proj (example.py:28,31; :57,59; :97,103), each a full GL draw
 * (src/alproj/project.py:276).  Here a render whose view (camera position and angles, fov,
 * w, h, offsets) equals the previous frame's on the same mesh and mask reuses that frame's
 * visibility buffer and runs only the resolve stage; value source, lens coefficients and
 * min_distance may differ.  Bit-identical to a full frame (the raster passes are
 * deterministic).  alp_mesh_frame_counts reports how many frames took each way:
 * counts[0] full, counts[1] resolve only. */
int alp_render_enqueue(alp_mesh_t *mesh, const double params[ALP_NPARAM],
                       const double *offsets, double min_distance);
int alp_render_fetch(alp_mesh_t *mesh, float *out);
int alp_mesh_frame_counts(alp_mesh_t *mesh, int64_t counts[2]);
/* Device time of the launches of the last alp_render_enqueue on this mesh (HIP events owned by the mesh, on the
 * library stream; waits for the frame). */
int alp_mesh_frame_ms(alp_mesh_t *mesh, float *ms);
/* Release the work areas the mesh keeps between calls of alp_render_rasterize_plan / alp_render_rasterize (the
 * compacted points and the 5 GB-class accumulator area of a 100 M-vertex frame); the mesh and its frame stay. */
int alp_mesh_trim(alp_mesh_t *mesh);
/* The last frame as h x w x 3 uint8: (image * scale) cast like numpy's astype(uint8)
 * (truncation toward zero, wrap), channels reversed when reverse_channels != 0 -- the tail of
 * sim_image(), src/alproj/project.py:322-324 (scale 255, RGB -> BGR), on the device, so that
 * 1 B instead of 4 B per channel cross PCIe. */
int alp_render_fetch_u8(alp_mesh_t *mesh, float scale, int reverse_channels, uint8_t *out);
/* The 64-bit visibility buffer of the last render, h x w, OpenGL window orientation (row 0 =
 * bottom), before the distortion remap: 0 = background, else (float32 bits of 1/depth) << 32 |
 * (0xFFFFFFFF - index of the winning triangle).  For inspection and parity tests. */
int alp_render_fetch_visibility(alp_mesh_t *mesh, uint64_t *out);

/* Post-processing of reverse_proj(), src/alproj/project.py:361-373, for a render whose
 * values are the vertices themselves (value == NULL): the pixels whose first channel (offset-
 * relative x) is > 0 (:369), in row-major order.  alp_render_valid_count returns their number
 * M; alp_render_fetch_valid then writes idx_out[M] (linear pixel index v * w + u) and
 * xyz_out[M][3] = (x, y, z) = channels (0, 2, 1) (:361) plus offsets[0], offsets[2],
 * offsets[1] (:370-373; NULL = no offsets), float64. */
/* Install a coordinate image produced elsewhere (h x w x 3 float32, row 0 = top: what persp_proj(vert,
 * vert, ...) returns, src/alproj/project.py:360) as the mesh's current frame, so that the
 * post-processing below runs on it as it would after alp_render_enqueue.  Its visibility buffer
 * is empty. */
int alp_render_load(alp_mesh_t *mesh, const float *image, int64_t h, int64_t w);
int alp_render_valid_count(alp_mesh_t *mesh, int64_t *count);
int alp_render_fetch_valid(alp_mesh_t *mesh, const double *offsets, uint32_t *idx_out, double *xyz_out);
/* The same survivors as three contiguous columns x_out[M], y_out[M], z_out[M] -- the layout a DataFrame keeps its
 * float64 columns in, so that the table of reverse_proj() is assembled without a transposing copy. */
int alp_render_fetch_valid_planes(alp_mesh_t *mesh, const double *offsets, uint32_t *idx_out, double *x_out,
                                  double *y_out, double *z_out);

/* The whole table of reverse_proj(), src/alproj/project.py:361-373, for the survivors of alp_render_valid_count (M rows, in
 * pixel order): index_out[M] = the table's labels (linear pixel index v * w + u: the reference filters a RangeIndex-ed frame),
 * u_out / v_out[M] = pixel column / row as int16 (:366), block_out = (3 + channels) contiguous float64 rows of M: x, y, z as
 * alp_render_fetch_valid_planes defines them, then the caller's image array[h][w][channels] (ALP_U8 / _U16 / _F32 / _F64, :364)
 * at each surviving pixel, cast to float64 -- the DataFrame's float64 block as pandas lays it out.  The array goes up
 * once (63 MB for a 5616 x 3744 photograph); the host no longer gathers, casts and divides 11.7 M rows on one core. */
int alp_render_fetch_valid_table(alp_mesh_t *mesh, const double *offsets, const void *array, int array_dtype,
                                 int64_t channels, int64_t *index_out, int16_t *u_out, int16_t *v_out, double *block_out);

/* set_gcp(), src/alproj/gcp.py:644-648, without the reverse_proj table: for n pixels (u[i], v[i])
 * of the last render (values = the vertices themselves) write xyz_out[i] = (x, y, z) as
 * alp_render_fetch_valid defines them, or NaN where the pixel lies outside the image or does
 * not see the surface (the rows the reference's left join + dropna removes). */
int alp_render_gather(alp_mesh_t *mesh, const int32_t *u, const int32_t *v, int64_t n,
                      const double *offsets, double *xyz_out);

/* filter_gcp_distance(), src/alproj/gcp.py:711-724: keep[i] = 1 for the rows of xyz[n][3] (x, y, z as alp_render_gather
 * writes them) without a NaN coordinate whose distance from camera[3] (params x, y, z) is >= min_distance and
 * <= max_distance, 0 otherwise.  A NaN bound is an absent one (the reference's None); the distance is formed as numpy
 * forms it (sqrt(dx**2 + dy**2 + dz**2), float64, no contraction), so the mask is the reference's.  Validation as
 * gcp.py:699-703 (negative minimum, maximum below minimum: ALP_EINVAL). */
int alp_distance_mask(const double *xyz, int64_t n, const double camera[3], double min_distance,
                      double max_distance, uint8_t *keep);

/* The arithmetic core of the reference's built-in matchers, src/alproj/gcp.py:55-70 (cv2.BFMatcher() -- NORM_L2 -- .knnMatch(des1,
 * des2, k=2), then Lowe's ratio test): for each of the n_query rows of `query` (des1, the photograph) the two nearest of the
 * n_train rows of `train` (des2, the simulated image) by brute force, exactly.  Rows are `len` values, contiguous: ALP_U8 (AKAZE),
 * or ALP_F32 holding the integers 0..255 (OpenCV's SIFT), cast to bytes on the device; a value that is no such integer (NaN
 * included) is ALP_EINVAL naming the lowest offending flat index, and nothing is computed.  Squared distances are exact integers
 * (int8 matrix cores, int32 accumulators); the order is (squared distance, train index): the lower index first on a tie.
 *   idx[n_query][2]    the nearest and the second nearest train row;
 *   dist2[n_query][2]  their squared distances;
 *   dist[n_query][2]   the correctly rounded float32 square root of (float) dist2: cv2's DMatch.distance;
 *   good[n_query]      (double) dist[0] < ratio * (double) dist[1]: the comparison of gcp.py:63 as Python evaluates it;
 *   n_good             the number of good rows.
 * Each output may be NULL.  splits: 0 = the launch plan's choice of how many ranges the train rows are divided into, > 0 forces it
 * (tests; the results do not depend on it).  info, may be NULL: query tile, train tile, splits used, padded len, workgroups,
 * device bytes of the call.  ALP_EINVAL before anything is uploaded: NULL inputs, len outside 1..512, n_train < 2, a ratio that
 * is not finite, splits above the number of train tiles, a padded array above 2^31 bytes.  n_query = 0: nothing happens. */
int alp_match_knn2(const void *query, int64_t n_query, const void *train, int64_t n_train, int len, int dtype,
                   double ratio, int splits, int32_t *idx, int32_t *dist2, float *dist, uint8_t *good,
                   int64_t *n_good, int64_t info[6]);

/* The geometric outlier filter that image_match runs on every set of matches, src/alproj/gcp.py:507-519 (_filter_geometric with
 * outlier_filter="fundamental", gcp.py:254-273).  cv2's USAC cannot be restated (its random stream, MAGSAC scoring), so this is an
 * algorithm of the library's own: H minimal samples of 8 matches, the normalised 8-point fundamental matrix of each, the inlier
 * count of each over all n matches, the best one refitted on its inliers.  Everything is float64.  p1[n][2] (the photograph) and
 * p2[n][2] (the simulated image) are pixel coordinates; F is row-major, 9 doubles, with b^T F a = 0 for a = (x1, y1, 1) and
 * b = (x2, y2, 1).  The error of a match under F is the measure of cv2's classic FM_RANSAC, the larger of the two squared
 * point-to-epipolar-line distances, evaluated in exactly this order without fused multiply-adds:
 *     l2_i = (F[i][0]*x1 + F[i][1]*y1) + F[i][2]      i = 0..2
 *     l1_j = (F[0][j]*x2 + F[1][j]*y2) + F[2][j]      j = 0..1
 *     s    = (x2*l2_0 + y2*l2_1) + l2_2
 *     e    = max(s*s / (l2_0*l2_0 + l2_1*l2_1), s*s / (l1_0*l1_0 + l1_1*l1_1))
 *     inlier  <=>  e <= threshold*threshold            (a NaN e is no inlier)
 * Caps of every entry point: 8 <= n <= 2^20, 1 <= H <= 2^20, H * n <= 2^35; a finite threshold >= 0; otherwise ALP_EINVAL before
 * anything is uploaded, as for NULL arrays, a sample index outside [0, n) and splits above the number of match tiles.
 *
 * alp_epipolar_samples: samples[H][8], every row 8 distinct indices in [0, n) from the counter-based generator of the CMA-ES
 *   sampler keyed by (seed, hypothesis, attempt); a repeat within the row is rejected and the next draw taken.  A function of
 *   (n, H, seed) alone.
 * alp_epipolar_solve8: F[H][9], the normalised 8-point solve of every sample: Hartley's normalisation formed once from all n
 *   points (centroid, mean distance sqrt 2), the null vector of the sample's 8 x 9 matrix, the smallest singular value of the
 *   3 x 3 matrix zeroed, T2^T F T1, unit Frobenius norm.  A sample whose matrix has rank below 8 (a repeated point), or whose F
 *   is not finite, gives 9 NaN.  The sign of F is not fixed.
 * alp_epipolar_score: counts[H], the number of inliers of every F (0 for a NaN F).  splits: 0 = the launch plan's choice of how
 *   many ranges the matches are divided into, > 0 forces it (tests; the counts do not depend on it).  info, may be NULL:
 *   hypothesis tile, match tile, splits used, workgroups, device bytes of the call, match tiles.
 * alp_epipolar_mask: mask[n] and err[n] (either may be NULL) of every match under one F.
 * alp_epipolar_ransac: the whole filter, enqueued at once with no host round trip between its stages.  samples: NULL = drawn
 *   from `seed` as alp_epipolar_samples draws them, else samples[H][8].  The hypothesis with the highest count is chosen, the
 *   lowest index on a tie.  Up to `refits` (0..8) times the 8-point solution is then fitted to all current inliers (the
 *   eigenvector of the smallest eigenvalue of the 9 x 9 sum over them, rank 2) and re-scored; it replaces the current F only when
 *   the count strictly grows, otherwise the loop stops.  F[9] and mask[n] (either may be NULL): the final F and its inliers.  When
 *   the chosen count is below 8, every mask entry is 1 (the reference keeps all matches when cv2 returns no mask, gcp.py:270-271).
 *   info[24], may be NULL: [0] chosen hypothesis, [1] its count, [2] the final count, [3] refits run, [4] refits kept, [5] 1 when
 *   all matches were kept for want of 8 inliers, [6] hypothesis tile, [7] match tile, [8] splits, [9] workgroups of the score,
 *   [10] device bytes, [11] workgroups of the refit's reductions, [12..19] the count of each refit run (-1: not run). */
int alp_epipolar_samples(int64_t n, int64_t H, uint64_t seed, int32_t *samples);
int alp_epipolar_solve8(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, double *F);
int alp_epipolar_score(const double *p1, const double *p2, int64_t n, const double *F, int64_t H, double threshold,
                       int splits, int32_t *counts, int64_t info[6]);
int alp_epipolar_mask(const double *p1, const double *p2, int64_t n, const double F[9], double threshold,
                      uint8_t *mask, double *err);
int alp_epipolar_ransac(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H,
                        uint64_t seed, double threshold, int refits, int splits, double F[9], uint8_t *mask,
                        int64_t info[24]);

/* The same filter with outlier_filter="essential", src/alproj/gcp.py:200-252 (cv2.findEssentialMat with K): minimal samples of 5
 * matches, the five-point solver on each (Nister's formulation with Stewenius' Gauss-Jordan step), up to 10 essential matrices a
 * sample.  K[3] = {f, cx, cy} serves both images, as the reference builds it (gcp.py:232-236).  Every matrix is scored, chosen and
 * reported as the pixel-space matrix F = K^-T E K^-1 at unit Frobenius norm, under the error expression above, so `threshold` is
 * in pixels.  The order of the operations, for a numpy restatement (no fused multiply-adds):
 *     r = 1 / f;  x' = (x - cx) * r,  y' = (y - cy) * r                       both images
 *     a = E K^-1:     a[i][0] = r*E[i][0],  a[i][1] = r*E[i][1],  a[i][2] = E[i][2] - r*(cx*E[i][0] + cy*E[i][1])
 *     F = K^-T a:     F[0][j] = r*a[0][j],  F[1][j] = r*a[1][j],  F[2][j] = a[2][j] - r*(cx*a[0][j] + cy*a[1][j])
 *     F /= sqrt(sum of F[i][j]^2 in row-major order)
 * Caps: 5 <= n <= 2^20, 1 <= H <= 2^20 / 10 (alp_epipolar_samples5: 2^20), 10 * H * n <= 2^35; f finite and > 0, cx and cy finite;
 * otherwise ALP_EINVAL before anything is uploaded, as for the refusals above.
 *
 * alp_epipolar_samples5: samples[H][5], rows of 5 distinct indices drawn as alp_epipolar_samples draws its rows of 8, keyed by
 *   (seed, hypothesis, attempt) but on a stream word of their own: the 8-wide rows of a seed do not depend on them.  A function
 *   of (n, H, seed) alone.
 * alp_epipolar_solve5: F[H][10][9] and nsol[H].  Per sample: the 5 x 9 epipolar matrix of the normalised points (a row is
 *   x2'x1' x2'y1' x2' y2'x1' y2'y1' y2' x1' y1' 1); its null space by Gaussian elimination with complete pivoting (the first
 *   largest entry in row-major order; a pivot at or below 1e-13 of the first one: rank below 5), null vector c = 0..3 having 1 at
 *   free column 5 + c, 0 at the other three free columns and the rest by back substitution summed from the left; E = x N0 + y N1
 *   + z N2 + N3; the ten cubics det E = 0 and 2 E E^T E - tr(E E^T) E = 0 over the monomials x^3 y^3 x^2y xy^2 x^2z x^2 y^2z
 *   y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1; Gauss-Jordan with row pivoting on the first ten columns; the rows of x^2z, x^2,
 *   y^2z, y^2, xyz, xy give B(z) (x, y, 1)^T = 0, and det B is a polynomial of degree 10 in z.  All its real roots are found, each
 *   to the last bit that bisection can decide: between two neighbouring real roots of a derivative the next lower derivative is
 *   monotone, so the roots of the k-th derivative bracket those of the (k-1)-th, from the linear one down to the polynomial
 *   itself, inside Cauchy's bound.  A root of even multiplicity is not found.  For each root, (x, y, 1) is the cross product of two
 *   rows of B(z) (of the three pairs the one with the largest third component), then up to three Gauss-Newton steps on the ten
 *   cubics in (x, y, z) (a step that does not shrink the residual ends them).  A solution whose cubics, taken at E of unit
 *   Frobenius norm, still exceed 5e-14 in Euclidean norm after the steps is dropped: the steps did not converge, and what they
 *   left is no essential matrix.  Then F as above.  The solutions of a sample stand in ascending order of the root z that
 *   bisection found, which means something only with respect to the null-space basis above.  The steps move z, so the
 *   polished z need not ascend, and two neighbouring roots may be taken to the same solution, which then fills two slots.
 *   The unused slots hold 9 NaN.  A sample of rank below 5 (a repeated point), a vanishing pivot or leading coefficient, a
 *   non-finite coefficient of the polynomial or any non-finite F gives 90 NaN and nsol 0.  The sign of F is not fixed.
 * alp_essential_ransac: alp_epipolar_ransac over the 10 * H slots of alp_epipolar_solve5, with these differences.  samples: NULL
 *   = drawn as alp_epipolar_samples5 draws them, else samples[H][5].  A NaN slot counts 0; info[0] is the chosen slot h * 10 + slot,
 *   the lowest on a tie.  The refit forms the 9 x 9 sum in the K-normalised coordinates x', y' above, so that its smallest
 *   eigenvector is K^T F K of the pixel-space fit; that matrix is projected onto the essential matrices (singular values (s, s, 0)
 *   with s the mean of the two largest) and taken back to pixels and to unit norm as above.  When the chosen count is below 5,
 *   which means that no sample gave a finite matrix, every mask entry is 1 and info[5] = 1.  The other info words are those of
 *   alp_epipolar_ransac; the launch plan is that of 10 * H hypotheses. */
int alp_epipolar_samples5(int64_t n, int64_t H, uint64_t seed, int32_t *samples);
int alp_epipolar_solve5(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H,
                        const double K[3], double *F, int32_t *nsol);
int alp_essential_ransac(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H,
                         uint64_t seed, const double K[3], double threshold, int refits, int splits, double F[9],
                         uint8_t *mask, int64_t info[24]);

/* The same two filters with ransac_method="LMEDS", src/alproj/gcp.py:160-279 (the argument at :160-161, handed to cv2 at :239-245
 * and :260-266): least median of squares (Rousseeuw 1984), which needs no threshold.  Not cv2's LMedS: an algorithm of the
 * library's own over the hypotheses, the error e and the refit defined above, so that numpy can restate it exactly.
 *     value of F     v = the rank-th smallest (rank is 1-based) of e over all n matches, a NaN e (and every e of a NaN F) counting
 *                    as +inf.  e is then a non-negative double or +inf, and such doubles order as their bit patterns do as
 *                    unsigned 64-bit integers: the device selects on the bits, exactly, and v is one of the e bit for bit.
 *     choice         the hypothesis (the slot h * 10 + slot) with the smallest v, the lowest index on a tie; a smallest v that is
 *                    not finite keeps every match (mask all 1, info[5] = 1) and runs no refit.
 *     bound          b2 = max(scale2 * v, floor2): one multiplication, then the larger; a match is an inlier iff e <= b2.
 *     refit          up to `refits` (0..8) times: the refit of alp_epipolar_ransac (alp_essential_ransac) on the inliers of the
 *                    current F at its bound, the value of the candidate; the candidate replaces the current F, and its value and
 *                    bound the current ones, only when its value is strictly smaller, otherwise the loop stops.  mask[n]: the
 *                    inliers of the final F at its own bound.
 * The caller forms rank, scale2 and floor2; the Python layer takes rank = min(n, max(m + 1, ceil(quantile * n))) with m = 8 (5),
 * scale2 = (2.5 * (1 / Phi^-1((1 + quantile) / 2)) * (1 + 5 / (n - m)))^2 (Rousseeuw and Leroy's robust standard deviation; 1.4826
 * at the median) and floor2 = min_threshold^2.  There is no threshold argument.
 * Caps: those of the sibling entry points, and passes * H * n <= 2^35 with passes = 16 (every pass of the select forms every error
 * again; the essential filter: 10 * H for H); rank in 1..n; scale2 and floor2 finite and >= 0; refits 0..8; otherwise ALP_EINVAL
 * before anything is uploaded, as for NULL arrays, a sample index outside [0, n) and splits above the number of match tiles.
 *
 * alp_epipolar_select: value[H], the rank-th smallest e of every F[H][9] (+inf for a NaN F).  A radix select on the bits of e, the
 *   most significant 4-bit digit first; no H x n array is formed and the result does not depend on splits (0 = the launch plan's
 *   choice, > 0 forces it).  info[8], may be NULL: hypothesis tile, match tile, splits used, workgroups, device bytes of the call,
 *   match tiles, passes, bytes of the partial histograms.
 * alp_epipolar_lmeds / alp_essential_lmeds: the whole filter, enqueued at once with no host round trip between its stages; samples,
 *   seed, K, F[9] and mask[n] as for alp_epipolar_ransac / alp_essential_ransac.  info[24], may be NULL, in alp_epipolar_ransac's
 *   layout with inlier counts at the bound of the matrix in question where the counts were: [0] chosen hypothesis (slot), [1] the
 *   inliers of the chosen F at its bound, [2] of the final F at its bound, [3] refits run, [4] refits kept, [5] 1 when all matches
 *   were kept, [6] hypothesis tile, [7] match tile, [8] splits, [9] workgroups of a pass of the select, [10] device bytes, [11]
 *   workgroups of the refit's reductions, [12..19] the inliers of each refit's candidate at the candidate's own bound (-1: not run;
 *   0 when its value is not finite), [20] passes of the select over the hypotheses, [21] passes of the select over the errors of
 *   one F, [22] match tiles, [23] bytes of the partial histograms.  stats[12], may be NULL: [0] the chosen value, [1] the final
 *   value, [2] the final b2, [3..10] the value of each refit's candidate (NaN: not run), [11] NaN.  When every match was kept,
 *   [0] = [1] = +inf and [2] is not meaningful. */
int alp_epipolar_select(const double *p1, const double *p2, int64_t n, const double *F, int64_t H, int64_t rank, int splits,
                        double *value, int64_t info[8]);
int alp_epipolar_lmeds(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                       int64_t rank, double scale2, double floor2, int refits, int splits, double F[9], uint8_t *mask,
                       int64_t info[24], double stats[12]);
int alp_essential_lmeds(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                        const double K[3], int64_t rank, double scale2, double floor2, int refits, int splits, double F[9],
                        uint8_t *mask, int64_t info[24], double stats[12]);

/* The spatial thinning of image_match, src/alproj/gcp.py:282-357 (_filter_spatial): mask[n] keeps one point per distinct value
 * of cell_id[n].  dist == NULL: the lowest index of each cell (selection="first").  Otherwise the lowest dist of each cell, the
 * lowest index on an equal dist (selection="center": pandas' idxmin); dist must be >= 0 and not NaN.  The table is indexed by
 * cell_id - min(cell_id): a span above 2^26 cells is ALP_EINVAL, as is n above 2^30.  n = 0: nothing happens. */
int alp_grid_thin(const int64_t *cell_id, const double *dist, int64_t n, uint8_t *mask);

/* Compute part of to_geotiff(), src/alproj/project.py:376-503 (the GeoTIFF file itself is
 * written by the caller): n points (x, y, values[n][nb]) -> uint8 raster out[nb][height][width].
 * Pixel of a point: col = int((x - x_min) / resolution), row = int((y_max - y) / resolution),
 * both clipped (:435-436); per band and pixel the aggregate `agg` of the points that fall in it,
 * NaN values skipped (:450-459); then `sweeps` passes in which every empty pixel takes the
 * NaN-aware aggregate of its 3x3 neighbourhood (:462-479; sweeps = ceil(max_dist / resolution),
 * 0 = no interpolation); empty pixels -> nodata, others clipped to [0, 255] and truncated
 * (:483-485). */
enum alp_agg { ALP_AGG_MEAN = 0, ALP_AGG_MAX = 1, ALP_AGG_MIN = 2, ALP_AGG_MEDIAN = 3 };
/* The same computation fed from the RESIDENT coordinate image of the last render (values = the
 * vertices themselves), i.e. reverse_proj() -> to_geotiff() back to back, example.py:103-106,
 * without the multi-million-row table in between:
 *   alp_render_rasterize_plan  selects the pixels that see the surface (x > 0,
 *       src/alproj/project.py:369), keeps their x = channel 0 + offsets[0], y = channel 2 +
 *       offsets[2] (:361, :370-373) on the device and returns their number and bounds[4] =
 *       x_min, y_min, x_max, y_max (:420-421) -- from which the caller derives width / height
 *       exactly as :422-425 does;
 *   alp_render_rasterize  takes the caller's image `array` (h x w x channels of the frame's size;
 *       ALP_U8, ALP_U16, ALP_F32 or ALP_F64 -- the table's float64 channel columns, :364-367),
 *       the channel index of each of the nb output bands, and rasterises like
 *       alp_rasterize_points.  The plan belongs to the frame it was made for. */
int alp_render_rasterize_plan(alp_mesh_t *mesh, const double *offsets, int64_t *n_valid, double bounds[4]);
int alp_render_rasterize(alp_mesh_t *mesh, const void *array, int array_dtype, int64_t channels,
                         const int32_t *band_channel, int64_t nb, double x_min, double y_max,
                         double resolution, int64_t width, int64_t height, int agg, int sweeps,
                         int nodata, uint8_t *out);
int alp_rasterize_points(const double *x, const double *y, const double *values, int64_t n, int64_t nb,
                         double x_min, double y_max, double resolution, int64_t width, int64_t height,
                         int agg, int sweeps, int nodata, uint8_t *out);
/* The float32 raster (nb, height, width) itself, after the sweeps and before the byte conversion (the reference's
 * `raster_data`, src/alproj/project.py:448-479; NaN = empty): what the parity tests compare with pandas bit for bit. */
int alp_rasterize_points_f32(const double *x, const double *y, const double *values, int64_t n, int64_t nb,
                             double x_min, double y_max, double resolution, int64_t width, int64_t height,
                             int agg, int sweeps, float *out);
/* The same with the band values as nb separate columns (columns[b][i]: each n contiguous doubles -- how a DataFrame keeps
 * them, so that to_geotiff(df) hands its columns over without the transposed copy df[bands].to_numpy() makes, ~100 ms for
 * 16 M rows x 3 bands); byte-valued columns (a photograph's bands, at most four) are packed into the sort's payload as they lie,
 * any others interleaved on the device. */
int alp_rasterize_columns(const double *x, const double *y, const double *const *columns, int64_t n, int64_t nb,
                          double x_min, double y_max, double resolution, int64_t width, int64_t height,
                          int agg, int sweeps, int nodata, uint8_t *out);

/* Image-space distortion remap alone: replaces distort(), src/alproj/project.py:111-143.
 * img/out: h x w x c float32 host images; coeffs: a1,a2,k1..k6,p1,p2,s1..s4. */
int alp_distort_image(const float *img, int64_t h, int64_t w, int64_t c,
                      const double coeffs[14], float *out);
/* The float32 source map of that remap alone: map_x, map_y (h x w each) = what distort() hands to
 * cv2.remap, src/alproj/project.py:128-140 (_distort of the pixel grid with 1/a1, 1/a2 and every other
 * coefficient negated, cast to float32). */
int alp_distort_map(int64_t h, int64_t w, const double coeffs[14], float *map_x, float *map_y);

#ifdef __cplusplus
}
#endif
#endif /* ALPROJ_HIP_H */
