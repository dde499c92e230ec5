// The point-set handle of alp_points.hip, shared with the device loop of the CMA-ES generation (alp_cma.hip), which feeds the
// population kernels from device-resident records.  Not part of the ABI.
#pragma once

#include <vector>

#include "alp_internal.h"

// ------------------------------------------------------------------ the handle
struct alp_points {
    int64_t n = 0;
    int64_t n_pad = 0;
    int precision = ALP_F32;
    double origin[3] = {0, 0, 0};
    // row length of a grid point set (rd.w > 0: the projection reads z alone and takes x, y from the first row / one value per
    // row; alp_points.hip: points_grid_detect); rd.w = 0: the plane path
    alp::RowDiv rd;
    // the planes live in at most three allocations (a hipMalloc / hipFree pair of this size costs ~1 ms: seven of them were a
    // third of what compute_residuals spent at 10 M points): coordinates at creation, observed pixels at alp_points_set_observed*,
    // projected pixels at the first alp_project
    alp::DeviceBuffer<> slab_xyz, slab_obs, slab_uv;
    void *x = nullptr, *y = nullptr, *z = nullptr;
    void *uo = nullptr, *vo = nullptr;
    void *u = nullptr, *v = nullptr;
    bool projected = false;
    // per-point frequency weights (alp_points_set_weights): one more plane of the set's element type, NULL = none set.  w_sum:
    // the float64 sum of the stored (rounded) weights in index order -- what the count slot of every reduction carries then
    alp::DeviceBuffer<> w;
    double w_sum = 0;
    double count_slot() const { return w ? w_sum : (double)n; }
    // the weight table (alp_points_set_weight_table): wt_rows rows of n weights of the set's element type, row r at r * n, and
    // behind them (256-byte aligned) the wt_rows float64 row sums the device formed -- one allocation, NULL = no table.
    // Independent of the plane above: a call that names table rows ignores `w`, every other call ignores the table.
    alp::DeviceBuffer<> wt;
    int wt_rows = 0;
    double *wt_sums = nullptr;
    // population-evaluation scratch
    int64_t cand_cap = 0;
    alp::DeviceBuffer<> cand_dev;
    alp::PinnedBuffer<> cand_host;
    alp::DeviceBuffer<double> partials;
    alp::DeviceBuffer<double> sums_dev;    // cand_cap + 1
    alp::PinnedBuffer<double> sums_host;   // cand_cap + 1
    int64_t last_info[3] = {0, 0, 0};     // alp_eval_population_info: variant, stripes, tile columns of the last launch
    int64_t pending_P = 0;
    int pending_loss = 0;
    double pending_f_scale = 0;
    std::vector<double> cand_copy;   // the P x 25 parameter vectors of the pending call (argmin confirmation)
    // last population evaluation: before the kernels, after them, after the all-reduce, after the mend pass
    alp::Event ev[4];
    bool timed = false;
    // argmin confirmation (float32 sets): the count word, float64 records, partial sums and sums of up to CONFIRM_MAX candidates
    alp::DeviceBuffer<> conf_dev;
    alp::PinnedBuffer<double> conf_host;   // CONFIRM_MAX + 1
    // the mend pass of a float32 set (alp_points_set_mend; alp_points.hip: mend_launch)
    bool mend = false;
    alp::DeviceBuffer<> mend_cnt;  // MendCount: the last pass's count and the total since mend was enabled
    alp::DeviceBuffer<> mend_dev;  // mend_cap x (index, mended sum, PoseRec<double>)
    int64_t mend_cap = 0;
    alp::DeviceBuffer<double> mend_params;   // the host path's cand_cap x 25 parameter rows (the device loop passes its own)
    bool mend_ran = false;         // the last population evaluation ran the pass
    int64_t mend_info[2] = {0, 0}; // its stripes and tile columns
    // device loops of the CMA-ES generation (alp_cma.hip) built on this set: told when it is destroyed; while one of them has
    // generations enqueued (loop_pending) they use the population scratch above, and an alp_eval_population_enqueue is refused
    std::vector<alp_cma_t *> loops;
    bool loop_pending = false;
    // device loops of the least-squares iteration (alp_lm.hip) built on this set: told when it is destroyed (they own their scratch)
    std::vector<alp_lm_t *> lm_loops;
    size_t esize() const { return precision == ALP_F64 ? 8 : 4; }
};

namespace alp {

// The population evaluation of P candidates whose pose records already lie in p->cand_dev (general records at [0, P), the
// lens-free ones at [cand_cap, cand_cap + P) when `lens_free`): grid choice (host/alp_plan.h: pop_grid), popeval_kernel + reduce_partials_kernel into
// p->sums_dev (P + 1 sums, the last one the vertex count), the all-reduce of those sums when a communicator exists, and
// last_info / the timing events.  Enqueue only.  The caller has reserved the scratch for P (points_pop_reserve).
// `batched` (the device loop's multi-start launch, K starts x P candidates): the stripe count is capped so that the partial sums
// (stripes x P doubles) stay within host::POP_BATCHED_PARTIALS_BYTES, and when the stripes alone do not fill the GPU (a GCP-sized set
// has a handful of rows) the grid gets candidate-tile columns up to four workgroups per CU.  Every other launch keeps its grid.
// `params_dev`: the P x 25 float64 parameter rows of the candidates on the device, which the mend pass folds again in float64 --
// needed when p->mend is set on a float32 set, unused otherwise.
int popeval_launch(alp_points *p, int64_t P, int loss_kind, double f_scale, bool lens_free, bool shared_pose, bool batched = false,
                   const double *params_dev = nullptr);
// population scratch (records, sums) for P candidates
int points_pop_reserve(alp_points *p, int64_t P);
// alp_points_destroy: a device loop built on the set loses it (its later calls return ALP_ESTATE)
void cma_points_gone(alp_cma_t *h);
void lm_points_gone(alp_lm_t *h);
// rounds of a least-squares device loop are enqueued and not yet waited for (they read the set's planes, the weights included)
bool lm_loop_pending(const alp_lm_t *h);

// One evaluation of the least-squares device loop (alp_lm.hip), normal_poses_kernel + reduce_normal_poses_kernel given the list:
// the normal equations of the starts in `list` (*count of them, in
// ascending order; running[k] != 0 for exactly those) under plans[k], over the fixed grid `g` = host::normal_batch_grid(n, K, cus):
// sums = K rows of T + 1 doubles in alp_normal_equations_batch's layout, zeros (and the point count) for a start that is not
// listed; all-reduced when a communicator exists.  partials: K * g.blocks * T doubles.  Enqueue only.
// `weight_rows` (alp_lm_create_rows): start k under row k of the set's weight table (the caller has checked that it has K rows),
// the count slot of row k = that row's sum.
int normal_listed_launch(alp_points *p, const JacPlan *plans, const int *list, const long long *count, const int *running, int K, int D,
                         const host::NormalGrid &g, int loss, double f_scale, double *partials, double *sums, bool weight_rows = false);

}  // namespace alp
