// libalproj_hip.so -- the device loop of the least-squares iteration (LsqOptimizer.optimize(method="normal", starts=K,
// device_loop=True)).
//
// The host lockstep (alproj_amd/optimize.py: normal_lm_batch) pays, per round, K host folds of a plan, an upload of K x 2.7 KB,
// two launches, a copy back, a synchronisation and K numpy state-machine steps with a Cholesky each; at GCP size the kernels
// are tens of microseconds of that.  Here the state of the K runs (host/alp_lm.h: LmState) lives on the device and a round is
// enqueued on the library stream with no copy and no synchronisation in between:
//   1. normal_poses_kernel + reduce_normal_poses_kernel on the list (alp_points.hip: normal_listed_launch), + the all-reduce of the
//      K (T + 1) sums when a communicator exists: the sums at the trial points of the starts that still run
//   2. lm_step_kernel     one workgroup of one wave per start: the two transitions of host/alp_lm.h on the start's sums, then --
//                         for a start that goes on -- the 25-parameter row (optimize.py _candidate_matrix) and its plan
//                         (host/alp_jacplan.h: lane 0 folds the pose, lane j < D the derivative for target j)
//   3. lm_select_kernel   one workgroup: the running starts in ascending order (ballot + prefix), their count, and a flag per
//                         start, in device memory
// alp_lm_create runs 2 (without a transition) and 3, so that the first round finds its trial points, plans and list.
// The state machine itself is the header's serial code, run by lane 0 on the start's state in LDS: the same statements as on
// the host (host/alp_host_selfcheck.cpp --lm), which is what tests/test_lm_device_host.py holds to _normal_lm_steps.
// This translation unit is compiled with -ffp-contract=off (alproj_amd/_build.py): the iteration follows numpy's operation
// order, one rounding per operation.  No atomics: every rank computes the same states from the all-reduced sums.
#include "alp_points_internal.h"

#include <cmath>

namespace {

using namespace alp;

constexpr int LM_MAX_STARTS = host::NORMAL_BATCH_MAX;      // 1024
constexpr int LM_ROW = LM_TRI + LM_MAX_D + 2;              // the longest row of sums

struct LmArgs {
    LmConfig cfg;
    double tmpl[ALP_NPARAM];
    double origin[3];
    double cost_scale;            // 0.5 f_scale^2: cost = cost_scale * sum rho, as Points.normal_equations forms it
    int32_t idx[LM_MAX_D];
    int32_t K;
};

// ------------------------------------------------------------------ 2. the step
// consume != 0: the running start blockIdx.x takes row blockIdx.x of `sums` (alp_normal_equations_batch's layout) through
// lm_advance.  Either way a start that (still) runs gets its parameter row's plan into plans[blockIdx.x].
__global__ __launch_bounds__(64) void lm_step_kernel(LmArgs a, LmState *__restrict__ states, const double *__restrict__ sums,
                                                     JacPlan *__restrict__ plans, int consume) {
    __shared__ LmState s_state;
    __shared__ JacPlan s_plan;
    __shared__ double s_row[LM_ROW];
    __shared__ double s_work[LM_WORK];
    __shared__ double s_prm[ALP_NPARAM];
    static_assert(sizeof(LmState) % 8 == 0 && sizeof(JacPlan) % 8 == 0, "copied as doubles");
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= a.K) return;
    LmState *gs = states + k;
    if (gs->phase == LM_STOPPED) return;                     // the same in every lane
    const int D = a.cfg.D, tri = D * (D + 1) / 2, T = tri + D + 1;
    constexpr int SW = (int)(sizeof(LmState) / 8), PW = (int)(sizeof(JacPlan) / 8);
    for (int t = lane; t < SW; t += 64) ((double *)&s_state)[t] = ((const double *)gs)[t];
    if (consume)
        for (int t = lane; t < T; t += 64) s_row[t] = sums[(int64_t)k * (T + 1) + t];
    for (int t = lane; t < PW; t += 64) ((double *)&s_plan)[t] = 0.0;
    __syncthreads();
    if (consume) {
        if (lane == 0) lm_advance(a.cfg, &s_state, s_row, s_row + tri, a.cost_scale * s_row[T - 1], s_work);
        __syncthreads();
        for (int t = lane; t < SW; t += 64) ((double *)gs)[t] = ((const double *)&s_state)[t];
    }
    if (s_state.phase == LM_STOPPED) return;
    // the parameter row of the trial point: the template with the targets' values (a target cannot repeat)
    if (lane < ALP_NPARAM) s_prm[lane] = a.tmpl[lane];
    __syncthreads();
    if (lane < D) s_prm[a.idx[lane]] = s_state.trial[lane];
    __syncthreads();
    if (lane == 0) jacobian_plan_head_hd(s_prm, a.origin, D, 1, &s_plan);
    __syncthreads();
    if (lane < D) jacobian_plan_target_hd(s_prm, a.origin, a.idx[lane], lane, &s_plan);
    __syncthreads();
    for (int t = lane; t < PW; t += 64) ((double *)(plans + k))[t] = ((const double *)&s_plan)[t];
}

// ------------------------------------------------------------------ 3. the selection
// list[0 .. *count) = the starts that have not stopped, ascending; running[k] = 1 for those, 0 for the others.
__global__ __launch_bounds__(256) void lm_select_kernel(const LmState *__restrict__ states, int K, int *__restrict__ list,
                                                        int *__restrict__ running, long long *__restrict__ count) {
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + tid;
        const bool on = k < K && states[k].phase != LM_STOPPED;
        const unsigned long long m = __ballot(on);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (on) list[off + __popcll(m & ((1ull << lane) - 1ull))] = k;
        if (k < K) running[k] = on ? 1 : 0;
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

}  // namespace

// ------------------------------------------------------------------ the handle
struct alp_lm {
    alp_points *pts = nullptr;
    LmArgs a{};
    int loss = 0;
    double f_scale = 1.0;
    host::NormalGrid grid{0, 0};  // host::normal_batch_grid(n, K, cus): fixed for the life of the handle
    DeviceBuffer<> dev;           // one allocation: states, plans, sums, partials, list, running, count
    LmState *st = nullptr;
    JacPlan *plans = nullptr;
    double *sums = nullptr, *partials = nullptr;
    int *list = nullptr, *running = nullptr;
    long long *count = nullptr;
    bool pending = false;         // rounds enqueued, alp_lm_wait not yet called
    bool weight_rows = false;     // alp_lm_create_rows: start k under row k of the set's weight table
    int T() const { return a.cfg.D * (a.cfg.D + 1) / 2 + a.cfg.D + 1; }
};

namespace alp {
void lm_points_gone(alp_lm_t *h) { h->pts = nullptr; }
bool lm_loop_pending(const alp_lm_t *h) { return h->pending; }
}  // namespace alp

namespace {

int usable(alp_lm *h, const char *what) {
    if (int rc = require_init()) return rc;
    if (!h) return fail(ALP_EINVAL, "%s: handle is NULL", what);
    if (h->pending) return fail(ALP_ESTATE, "%s: rounds are enqueued; call alp_lm_wait first", what);
    return ALP_OK;
}

// step (with or without a transition) and selection, enqueued
int launch_step_select(alp_lm *h, int consume) {
    hipStream_t st = ctx().stream;
    hipLaunchKernelGGL(lm_step_kernel, dim3((unsigned)h->a.K), dim3(64), 0, st, h->a, h->st, (const double *)h->sums, h->plans, consume);
    hipLaunchKernelGGL(lm_select_kernel, dim3(1), dim3(256), 0, st, (const LmState *)h->st, (int)h->a.K, h->list, h->running, h->count);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

// alp_lm_create and, with `weight_rows`, alp_lm_create_rows
int lm_create(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
              const double *upper, const double *X0, int K, int loss, double f_scale, double ftol, double xtol, double gtol,
              int64_t max_nfev, bool weight_rows, alp_lm_t **out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(out, "out is NULL");
    *out = nullptr;
    ALP_REQUIRE(pts && tmpl && lower && upper && X0, "NULL argument");
    if (int rc = jacobian_targets_check(target_idx, D)) return rc;
    ALP_REQUIRE(K >= 1 && K <= LM_MAX_STARTS, "K must be 1..1024");
    ALP_REQUIRE(loss >= ALP_NORMAL_LINEAR && loss <= ALP_NORMAL_CAUCHY, "unknown loss");
    ALP_REQUIRE(f_scale > 0 && std::isfinite(f_scale), "f_scale must be a positive finite number");
    ALP_REQUIRE(max_nfev >= 1 && max_nfev <= INT32_MAX, "max_nfev must be 1..2^31-1");
    ALP_REQUIRE(!(ftol != ftol) && !(xtol != xtol) && !(gtol != gtol), "a tolerance is NaN");
    for (int i = 0; i < D; ++i) ALP_REQUIRE(!(lower[i] != lower[i]) && !(upper[i] != upper[i]) && lower[i] <= upper[i], "bounds must satisfy lower <= upper");
    if (!pts->uo) return fail(ALP_ESTATE, "alp_lm_create: observed uv not set");
    if (weight_rows && !pts->wt) return fail(ALP_ESTATE, "alp_lm_create_rows: no weight table set");
    if (weight_rows && pts->wt_rows != K)
        return fail(ALP_EINVAL, "alp_lm_create_rows: the weight table has %d rows, the loop %d starts: start k runs under row k", pts->wt_rows, K);
    alp_lm *h = new alp_lm();
    h->pts = pts;
    h->weight_rows = weight_rows;
    h->loss = loss;
    h->f_scale = f_scale;
    memset(&h->a, 0, sizeof(h->a));
    h->a.cfg.D = D;
    h->a.cfg.max_nfev = (int32_t)max_nfev;
    h->a.cfg.ftol = ftol;
    h->a.cfg.xtol = xtol;
    h->a.cfg.gtol = gtol;
    for (int i = 0; i < D; ++i) {
        h->a.cfg.lower[i] = lower[i];
        h->a.cfg.upper[i] = upper[i];
        h->a.idx[i] = target_idx[i];
    }
    for (int k = 0; k < ALP_NPARAM; ++k) h->a.tmpl[k] = tmpl[k];
    memcpy(h->a.origin, pts->origin, sizeof(h->a.origin));
    h->a.cost_scale = 0.5 * f_scale * f_scale;
    h->a.K = K;
    h->grid = host::normal_batch_grid(pts->n, K, ctx().cu_count);
    const int T = h->T();
    const size_t sz_state = round_up((int64_t)K * sizeof(LmState), 256), sz_plan = round_up((int64_t)K * sizeof(JacPlan), 256),
                 sz_sums = round_up((int64_t)K * (T + 1) * 8, 256), sz_part = round_up((int64_t)K * h->grid.blocks * T * 8 + 8, 256),
                 sz_int = round_up((int64_t)K * 4, 256);
    int rc = h->dev.reserve(sz_state + sz_plan + sz_sums + sz_part + 2 * sz_int + 256);
    if (!rc) {
        char *q = (char *)h->dev;
        h->st = (LmState *)q; q += sz_state;
        h->plans = (JacPlan *)q; q += sz_plan;
        h->sums = (double *)q; q += sz_sums;
        h->partials = (double *)q; q += sz_part;
        h->list = (int *)q; q += sz_int;
        h->running = (int *)q; q += sz_int;
        h->count = (long long *)q;
        std::vector<LmState> s((size_t)K);
        for (int k = 0; k < K; ++k) lm_start(h->a.cfg, X0 + (size_t)k * D, &s[(size_t)k]);
        hipStream_t st = ctx().stream;
        if (hipMemcpyAsync(h->st, s.data(), (size_t)K * sizeof(LmState), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemsetAsync(h->sums, 0, sz_sums, st) != hipSuccess)
            rc = fail(ALP_EHIP, "alp_lm_create: state upload failed");
        if (!rc) rc = launch_step_select(h, 0);
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(ALP_EHIP, "alp_lm_create: the first step failed");      // s (host) must outlive its copy
    }
    if (rc) {
        delete h;
        return rc;
    }
    pts->lm_loops.push_back(h);
    *out = h;
    return ALP_OK;
}

}  // namespace

extern "C" {

int alp_lm_create(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                  const double *upper, const double *X0, int K, int loss, double f_scale, double ftol, double xtol, double gtol,
                  int64_t max_nfev, alp_lm_t **out) {
    return lm_create(pts, tmpl, target_idx, D, lower, upper, X0, K, loss, f_scale, ftol, xtol, gtol, max_nfev, false, out);
}

int alp_lm_create_rows(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                       const double *upper, const double *X0, int K, int loss, double f_scale, double ftol, double xtol, double gtol,
                       int64_t max_nfev, alp_lm_t **out) {
    return lm_create(pts, tmpl, target_idx, D, lower, upper, X0, K, loss, f_scale, ftol, xtol, gtol, max_nfev, true, out);
}

int alp_lm_destroy(alp_lm_t *h) {
    if (!h) return ALP_OK;
    if (ctx().ready) hipStreamSynchronize(ctx().stream);
    if (h->pts) {
        auto &v = h->pts->lm_loops;
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] == h) {
                v.erase(v.begin() + (long)i);
                break;
            }
    }
    delete h;
    return ALP_OK;
}

int alp_lm_run(alp_lm_t *h, int64_t rounds) {
    if (int rc = usable(h, "alp_lm_run")) return rc;
    ALP_REQUIRE(rounds >= 0, "rounds is negative");
    alp_points *p = h->pts;
    if (!p) return fail(ALP_ESTATE, "alp_lm_run: the point set of this device loop has been destroyed");
    if (h->weight_rows && p->wt_rows != h->a.K)
        return fail(ALP_ESTATE, "alp_lm_run: the weight table of the point set no longer has the loop's %d rows", (int)h->a.K);
    if (rounds == 0) return ALP_OK;
    h->pending = true;                   // from the first launch on: a failure below still needs alp_lm_wait
    for (int64_t r = 0; r < rounds; ++r) {
        if (int rc = normal_listed_launch(p, h->plans, h->list, h->count, h->running, h->a.K, h->a.cfg.D, h->grid, h->loss, h->f_scale,
                                          h->partials, h->sums, h->weight_rows))
            return rc;
        if (int rc = launch_step_select(h, 1)) return rc;
    }
    return ALP_OK;
}

int alp_lm_wait(alp_lm_t *h, int64_t *pending) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(h, "handle is NULL");
    if (!h->pending) return fail(ALP_ESTATE, "alp_lm_wait: nothing enqueued");
    h->pending = false;
    long long count = 0;
    ALP_HIP(hipMemcpyAsync(&count, h->count, sizeof(count), hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    if (pending) *pending = (int64_t)count;
    return ALP_OK;
}

int alp_lm_get(alp_lm_t *h, double *x, double *cost, double *grad_norm, int64_t *iterations, int64_t *evaluations, int32_t *status,
               double *trial, double *mu, double *nu) {
    if (int rc = usable(h, "alp_lm_get")) return rc;
    const int K = h->a.K, D = h->a.cfg.D;
    std::vector<LmState> s((size_t)K);
    ALP_HIP(hipMemcpyAsync(s.data(), h->st, (size_t)K * sizeof(LmState), hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    for (int k = 0; k < K; ++k) {
        const LmState &r = s[(size_t)k];
        for (int i = 0; i < D; ++i) {
            if (x) x[(size_t)k * D + i] = r.x[i];
            if (trial) trial[(size_t)k * D + i] = r.trial[i];
        }
        if (cost) cost[k] = r.cost;
        if (grad_norm) grad_norm[k] = r.nfev >= 1 ? lm_grad_norm(h->a.cfg, &r) : NAN;
        if (iterations) iterations[k] = r.iterations;
        if (evaluations) evaluations[k] = r.nfev;
        if (status) status[k] = r.status;
        if (mu) mu[k] = r.mu;
        if (nu) nu[k] = r.nu;
    }
    return ALP_OK;
}

int alp_lm_step_host(alp_lm_t *h, const double *sums) {
    if (int rc = usable(h, "alp_lm_step_host")) return rc;
    ALP_REQUIRE(sums, "sums is NULL");
    hipStream_t st = ctx().stream;
    ALP_HIP(hipMemcpyAsync(h->sums, sums, (size_t)h->a.K * (h->T() + 1) * 8, hipMemcpyHostToDevice, st));
    if (int rc = launch_step_select(h, 1)) return rc;
    ALP_HIP(hipStreamSynchronize(st));
    return ALP_OK;
}

}  // extern "C"
