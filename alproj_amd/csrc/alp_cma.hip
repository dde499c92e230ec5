// libalproj_hip.so -- the device loop of the CMA-ES generation (CMAOptimizer.optimize(..., device_loop=True)).
//
// The reference's generation (src/alproj/optimize.py:410-427: ask x population_size, evaluate, tell) runs on the host
// in the default path of the product: numpy sampling, the candidate matrix, a fold of every pose, one population
// evaluation with its synchronisation and copy back, and numpy's tell with an eigendecomposition.  At the reference's
// own size (1127 GCPs, pop 50, D 9) three quarters of a generation were that host work.  Here the state of the optimiser
// (mean, sigma, C = B D^2 B^T, p_sigma, pc, g) lives on the device and a generation is three launches on the library
// stream, with no copy to the host and no synchronisation between generations:
//   1. cma_generation_kernel   the draw of alp_cma_sample (alp_sampler.h, the same bits) from the DEVICE state, the
//                              de-normalisation x * (upper - lower) + lower, the scatter into the 25-vector template
//                              (optimize.py:341-350, _candidate_matrix) and the fold of every pose (host/alp_fold.h)
//                              into the records the population kernels read
//   2. popeval_kernel + reduce_partials_kernel (alp_points.hip: popeval_launch), + the all-reduce of the sums when a
//                              communicator exists
//   3. cma_tell_kernel         one workgroup: losses = sums / n_total, the stable ascending order (NaN as +inf), the
//                              update of cma.py:tell_population in its order, then the next generation's _eigen step
//                              (symmetrise, eigendecomposition by parallel cyclic Jacobi warm-started from the previous B,
//                              clamp, C = B diag(d^2) B^T, BD)
// This translation unit is compiled with -ffp-contract=off (alproj_amd/_build.py): the de-normalisation and the update
// follow numpy's operation order, one rounding per operation.  Every rank runs the same replica: the sums are all-reduced,
// the tell is one workgroup without atomics, so every rank computes the same state.
// Multi-start (alp_cma_create_starts, CMAOptimizer.optimize(..., starts=K)): K independent states share the three launches of a
// generation.  Candidate k * P + i of the draw is draw i of start k (start k's seed, state and generation: the bits of
// alp_cma_sample(..., seeds[k], g)), the evaluation runs K * P candidates, and the tell is K workgroups, workgroup k on start k's
// losses sums[k * P .. k * P + P) / sums[K * P], its state and its slice of the scratch.
#include "alp_points_internal.h"
#include "alp_sampler.h"

#include <cmath>

namespace {

using namespace alp;

constexpr int CMA_MAX_D = SAMPLER_MAX_D;      // 32
constexpr int CMA_MAX_P = 4096;
constexpr int CMA_MAX_STARTS = 1024;
constexpr int64_t CMA_MAX_TOTAL = 65536;    // K * P
constexpr int TELL_THREADS = 256;
constexpr int JACOBI_MAX_SWEEPS = 40;
constexpr double CMA_EPS = 1e-8;             // cma.py _EPS
constexpr double CMA_SIGMA_MAX = 1e32;       // cma.py _SIGMA_MAX

// the optimiser's state, float64, on the device
struct CmaState {
    double mean[CMA_MAX_D], ps[CMA_MAX_D], pc[CMA_MAX_D], d[CMA_MAX_D];
    double C[CMA_MAX_D * CMA_MAX_D], B[CMA_MAX_D * CMA_MAX_D];     // rows of D
    double BD[CMA_MAX_D * CMA_MAX_D];                              // B diag(d), rows of dmax columns, zero-padded (make_x)
    double sigma;
    long long g;
    unsigned k0, k1;                                               // the sampler's key: this start's seed
};

// the constants of cma.py:CMA.__init__, as the host object computed them (nothing is recomputed here)
struct CmaHyper {
    int D, P, mu, dmax, K;
    double mu_eff, c1, cmu, cc, c_sigma, d_sigma, chi_n, cm, sum_w;
};

// the candidate matrix and the fold: template (params_init as a 25-vector), target columns and their bounds
struct ExpandArgs {
    double tmpl[ALP_NPARAM];
    double lo[CMA_MAX_D], hi[CMA_MAX_D];
    int idx[CMA_MAX_D];
    double origin[3];
};

// ------------------------------------------------------------------ 1. sample + expand + fold
// cma_sample_kernel (alp_sampler.hip) with mean, sigma and the generation counter taken from the device state; the lane
// that holds the accepted draw then de-normalises, scatters and folds its candidate.
// K starts: candidate `cand` of the grid is draw i = cand % P of start cand / P, from start k's state and key.
template <typename T, int DMAX, bool LF>
__global__ __launch_bounds__(256) void cma_generation_kernel(SamplerArgs a0, ExpandArgs e, const CmaState *__restrict__ states, long long P,
                                                             long long total, double *__restrict__ x_out, double *__restrict__ cand_out,
                                                             PoseRec<T> *__restrict__ recs, long long lf_off) {
    const long long cand = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (cand >= total) return;
    const long long start = cand / P, draw = cand - start * P;
    const CmaState *st = states + start;
    const int lane = (int)(threadIdx.x & 63);
    SamplerArgs a = a0;
#pragma unroll
    for (int i = 0; i < DMAX; ++i)
        if (i < a.D) a.mean[i] = st->mean[i];
    a.sigma = st->sigma;
    a.gen = (unsigned)st->g;
    a.k0 = st->k0;
    a.k1 = st->k1;
    const double *BD = st->BD;
    double z[DMAX], x[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; ++j) z[j] = 0.0;
    int accepted = -1;
    for (int base = 0; base < a.n_max && accepted < 0; base += 64) {
        const int t = base + lane;
        bool ok = false;
        if (t < a.n_max) {
            draw_normals<DMAX>(z, a.D, (unsigned)t, (unsigned)draw, a.gen, a.k0, a.k1);
            ok = make_x<DMAX, false>(a, BD, z, x);
        }
        const unsigned long long m = __ballot(ok);
        if (m) accepted = base + __ffsll((long long)m) - 1;
    }
    const int t_final = accepted >= 0 ? accepted : a.n_max;
    if (lane != (t_final & 63)) return;
    draw_normals<DMAX>(z, a.D, (unsigned)t_final, (unsigned)draw, a.gen, a.k0, a.k1);
    make_x<DMAX, true>(a, BD, z, x);
    double prm[ALP_NPARAM];
    for (int k = 0; k < ALP_NPARAM; ++k) prm[k] = e.tmpl[k];
#pragma unroll
    for (int i = 0; i < DMAX; ++i)
        if (i < a.D) {
            double xi = x[i];
            if (accepted < 0 && a.bounded) xi = fmin(fmax(xi, a.lower[i]), a.upper[i]);
            x_out[cand * a.D + i] = xi;
            prm[e.idx[i]] = xi * (e.hi[i] - e.lo[i]) + e.lo[i];      // optimize.py _proj_error: x * (upper - lower) + lower
                                                                    // (a target named twice: the last one wins, as in numpy)
        }
    for (int k = 0; k < ALP_NPARAM; ++k) cand_out[cand * ALP_NPARAM + k] = prm[k];
    double g[POSE_WORDS];
    fold_pose_hd(prm, e.origin, g);
    for (int k = 0; k < POSE_WORDS; ++k) recs[cand].v[k] = (T)g[k];
    if (LF) {
        double lf[POSE_WORDS];
        lens_free_from_general_hd(g, lf);
        for (int k = 0; k < POSE_WORDS; ++k) recs[lf_off + cand].v[k] = (T)lf[k];
    }
}

// ------------------------------------------------------------------ 3. tell + eigen (one workgroup)
// Round `r` of the circle schedule of m (even) indices: pair k of m / 2.  Every unordered pair appears once in m - 1 rounds.
__device__ __forceinline__ void circle_pair(int m, int r, int k, int *p, int *q) {
    const int a = k == 0 ? m - 1 : (r + k) % (m - 1);
    const int b = (r - k + (m - 1)) % (m - 1);
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// C (LDS, D x D, symmetric) -> its eigenvectors as columns of B (LDS, holds the previous B on entry: the warm start) and
// its eigenvalues d2[]; A, A2, V, V2 are LDS scratch.  Parallel cyclic Jacobi: each round rotates D / 2 disjoint pairs
// at once (Rutishauser's formulas, Numerical Recipes' skip test), A <- P^T A P and V <- V P in one pass.
__device__ void jacobi_eigen(int D, double *C, double *B, double *d2, double *A, double *A2, double *V, double *V2, double *self_,
                             double *oth, double *dlt, int *partner, int *rotated, int *nrot) {
    const int tid = threadIdx.x;
    const int DD = D * D;
    // re-orthonormalise the warm start (one Newton-Schulz step, B <- B (3 I - B^T B) / 2: the rounding of B = B_old V would
    // otherwise accumulate over the generations)
    for (int e = tid; e < DD; e += blockDim.x) {
        const int i = e / D, j = e % D;
        double s = 0;
        for (int k = 0; k < D; ++k) s += B[k * D + i] * B[k * D + j];
        A2[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < DD; e += blockDim.x) {
        const int i = e / D, j = e % D;
        double s = 0;
        for (int k = 0; k < D; ++k) s += B[i * D + k] * ((k == j ? 1.5 : 0.0) - 0.5 * A2[k * D + j]);
        V2[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < DD; e += blockDim.x) B[e] = V2[e];
    __syncthreads();
    // A = B^T C B (symmetric by construction: the upper triangle is mirrored), V = I
    for (int e = tid; e < DD; e += blockDim.x) {
        const int i = e / D, j = e % D;
        double s = 0;
        for (int k = 0; k < D; ++k) s += C[i * D + k] * B[k * D + j];
        A2[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < DD; e += blockDim.x) {
        const int i = e / D, j = e % D;
        if (i <= j) {
            double s = 0;
            for (int k = 0; k < D; ++k) s += B[k * D + i] * A2[k * D + j];
            A[i * D + j] = s;
            A[j * D + i] = s;
        }
        V[e] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    const int m = (D + 1) & ~1;
    for (int sweep = 0; sweep < JACOBI_MAX_SWEEPS && m >= 2; ++sweep) {
        if (tid == 0) *nrot = 0;
        __syncthreads();
        for (int r = 0; r < m - 1; ++r) {
            if (tid < m / 2) {
                int p, q;
                circle_pair(m, r, tid, &p, &q);
                if (q < D) {
                    const double app = A[p * D + p], aqq = A[q * D + q], apq = A[p * D + q];
                    const double g = 100.0 * fabs(apq);
                    double c = 1.0, s = 0.0, t = 0.0;
                    const bool rot = apq != 0.0 && !(fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq));
                    if (rot) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        if (fabs(theta) > 1e150) t = 0.5 / theta;
                        else {
                            t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                            if (theta < 0) t = -t;
                        }
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        *nrot = 1;
                    }
                    partner[p] = q; partner[q] = p;
                    self_[p] = c; self_[q] = c;
                    oth[p] = -s; oth[q] = s;                  // P(q, p) = -s, P(p, q) = s
                    dlt[p] = -t * apq; dlt[q] = t * apq;
                    rotated[p] = rotated[q] = rot;
                } else if (p < D) {                            // paired with the padding index
                    partner[p] = p; self_[p] = 1.0; oth[p] = 0.0; dlt[p] = 0.0; rotated[p] = 0;
                }
            }
            __syncthreads();
            for (int e = tid; e < DD; e += blockDim.x) {
                const int i = e / D, j = e % D;
                double v;
                if (i == j) v = A[e] + dlt[i];
                else if (partner[i] == j && rotated[i]) v = 0.0;
                else {
                    const int lo = i < j ? i : j, hi = i < j ? j : i;
                    const int plo = partner[lo], phi = partner[hi];
                    v = self_[hi] * A[lo * D + hi];
                    if (oth[hi] != 0.0) v += oth[hi] * A[lo * D + phi];
                    v *= self_[lo];
                    if (oth[lo] != 0.0) {
                        double w = self_[hi] * A[plo * D + hi];
                        if (oth[hi] != 0.0) w += oth[hi] * A[plo * D + phi];
                        v += oth[lo] * w;
                    }
                }
                A2[e] = v;
                double u = V[i * D + j] * self_[j];
                if (oth[j] != 0.0) u += V[i * D + partner[j]] * oth[j];
                V2[e] = u;
            }
            __syncthreads();
            for (int e = tid; e < DD; e += blockDim.x) {
                A[e] = A2[e];
                V[e] = V2[e];
            }
            __syncthreads();
        }
        if (*nrot == 0) break;
        __syncthreads();
    }
    // B <- B V, eigenvalues on the diagonal
    for (int e = tid; e < DD; e += blockDim.x) {
        const int i = e / D, j = e % D;
        double s = 0;
        for (int k = 0; k < D; ++k) s += B[i * D + k] * V[k * D + j];
        V2[e] = s;
    }
    for (int i = tid; i < D; i += blockDim.x) d2[i] = A[i * D + i];
    __syncthreads();
    for (int e = tid; e < DD; e += blockDim.x) B[e] = V2[e];
    __syncthreads();
}

// TELL: one tell_population on the candidates X (P x D) with losses sums[i] / sums[K P] (vals == NULL) or vals[i];
// then (always) cma.py:_eigen on the state's C.  loss_out / order_out: the losses used and the stable ascending order.
// Workgroup k works on start k: its state and its P rows of X, sums, vals, loss_out, order_out, ys and wio (the order holds
// indices 0 .. P-1 within the start); sums[h.K * P] is the vertex count every start divides by.
template <bool TELL>
__global__ __launch_bounds__(TELL_THREADS) void cma_tell_kernel(CmaHyper h, CmaState *__restrict__ states, const double *__restrict__ weights,
                                                                const double *__restrict__ X_all, const double *__restrict__ sums_all,
                                                                const double *__restrict__ vals_all, double *__restrict__ loss_all,
                                                                int *__restrict__ order_all, double *__restrict__ ys_all,
                                                                double *__restrict__ wio_all) {
    const long long k = blockIdx.x, kP = k * h.P, kPD = kP * h.D;
    CmaState *__restrict__ st = states + k;
    const double *__restrict__ X = X_all + kPD;
    const double *__restrict__ sums = sums_all ? sums_all + kP : nullptr;
    const double n_total = sums_all ? sums_all[(long long)h.K * h.P] : 0.0;
    const double *__restrict__ vals = vals_all ? vals_all + kP : nullptr;
    double *__restrict__ loss_out = loss_all + kP;
    int *__restrict__ order_out = order_all + kP;
    double *__restrict__ ys = ys_all + kPD;
    double *__restrict__ wio = wio_all + kP;
    constexpr int M = CMA_MAX_D * CMA_MAX_D;
    __shared__ double C[M], B[M], A[M], A2[M], V[M], V2[M];
    __shared__ double mean[CMA_MAX_D], d[CMA_MAX_D], yw[CMA_MAX_D], ps[CMA_MAX_D], pc[CMA_MAX_D], d2[CMA_MAX_D];
    __shared__ double self_[CMA_MAX_D], oth[CMA_MAX_D], dlt[CMA_MAX_D];
    __shared__ int partner[CMA_MAX_D], rotated[CMA_MAX_D];
    __shared__ int nrot;
    __shared__ double sig, hsig;
    const int tid = threadIdx.x, D = h.D, P = h.P, DD = D * D;
    for (int e = tid; e < DD; e += blockDim.x) {
        C[e] = st->C[e];
        B[e] = st->B[e];
    }
    for (int i = tid; i < D; i += blockDim.x) {
        mean[i] = st->mean[i];
        d[i] = st->d[i];
        ps[i] = st->ps[i];
        pc[i] = st->pc[i];
    }
    if (tid == 0) sig = st->sigma;
    __syncthreads();
    if (TELL) {
        const long long g = st->g + 1;                       // self._g += 1
        // losses (host/alp_host.h losses_and_argmin: sums[i] / n_total) and the order of np.argsort(where(isnan, inf, l), kind="stable")
        for (int i = tid; i < P; i += blockDim.x) loss_out[i] = vals ? vals[i] : sums[i] / n_total;
        __syncthreads();
        for (int i = tid; i < P; i += blockDim.x) {
            double ki = loss_out[i];
            if (ki != ki) ki = INFINITY;
            int r = 0;
            for (int j = 0; j < P; ++j) {
                double kj = loss_out[j];
                if (kj != kj) kj = INFINITY;
                r += (kj < ki) || (kj == ki && j < i);
            }
            order_out[r] = i;
        }
        __syncthreads();
        // y_k = (x_k - mean) / sigma in sorted order
        const double sigma = sig;
        for (int e = tid; e < P * D; e += blockDim.x) {
            const int r = e / D, j = e % D;
            ys[e] = (X[(long long)order_out[r] * D + j] - mean[j]) / sigma;
        }
        __syncthreads();
        // y_w = sum over the mu best of y_k * w_k; mean += cm * sigma * y_w
        for (int j = tid; j < D; j += blockDim.x) {
            double s = 0.0;
            for (int r = 0; r < h.mu; ++r) s = s + ys[(long long)r * D + j] * weights[r];
            yw[j] = s;
        }
        __syncthreads();
        const double cs = h.c_sigma, cmsig = h.cm * sigma;
        // C^-1/2 = (B / d) B^T  (into A)
        for (int e = tid; e < DD; e += blockDim.x) {
            const int i = e / D, j = e % D;
            double s = 0.0;
            for (int k = 0; k < D; ++k) s += (B[i * D + k] / d[k]) * B[j * D + k];
            A[e] = s;
        }
        for (int j = tid; j < D; j += blockDim.x) mean[j] = mean[j] + cmsig * yw[j];
        __syncthreads();
        const double sq_ps = sqrt(cs * (2.0 - cs) * h.mu_eff);
        for (int i = tid; i < D; i += blockDim.x) {
            double s = 0.0;
            for (int k = 0; k < D; ++k) s += A[i * D + k] * yw[k];
            ps[i] = (1.0 - cs) * ps[i] + sq_ps * s;
        }
        __syncthreads();
        if (tid == 0) {
            double nn = 0.0;
            for (int k = 0; k < D; ++k) nn += ps[k] * ps[k];
            const double norm_ps = sqrt(nn);
            double s2 = sig * exp((cs / h.d_sigma) * (norm_ps / h.chi_n - 1.0));
            sig = s2 < CMA_SIGMA_MAX ? s2 : CMA_SIGMA_MAX;
            const double h_left = norm_ps / sqrt(1.0 - pow(1.0 - cs, (double)(2 * (g + 1))));
            const double h_right = (1.4 + 2.0 / (double)(D + 1)) * h.chi_n;
            hsig = h_left < h_right ? 1.0 : 0.0;
        }
        __syncthreads();
        const double h_sigma = hsig, cc = h.cc;
        const double sq_pc = h_sigma * sqrt(cc * (2.0 - cc) * h.mu_eff);
        for (int i = tid; i < D; i += blockDim.x) pc[i] = (1.0 - cc) * pc[i] + sq_pc * yw[i];
        // w_io = w * (w >= 0 ? 1 : D / (|C^-1/2 y_k|^2 + eps))
        for (int r = tid; r < P; r += blockDim.x) {
            const double wr = weights[r];
            if (wr >= 0) {
                wio[r] = wr * 1.0;
            } else {
                double nn = 0.0;
                for (int i = 0; i < D; ++i) {
                    double s = 0.0;
                    for (int k = 0; k < D; ++k) s += ys[(long long)r * D + k] * A[i * D + k];
                    nn += s * s;
                }
                const double nrm = sqrt(nn);
                wio[r] = wr * ((double)D / (nrm * nrm + CMA_EPS));
            }
        }
        __syncthreads();
        const double delta_h = (1.0 - h_sigma) * cc * (2.0 - cc);
        const double c1 = h.c1, cmu = h.cmu;
        const double coef = 1.0 + c1 * delta_h - c1 - cmu * h.sum_w;
        for (int e = tid; e < DD; e += blockDim.x) {
            const int i = e / D, j = e % D;
            double rmu = 0.0;
            for (int r = 0; r < P; ++r) rmu += (ys[(long long)r * D + i] * wio[r]) * ys[(long long)r * D + j];
            A2[e] = coef * C[e] + c1 * (pc[i] * pc[j]) + cmu * rmu;
        }
        __syncthreads();
        for (int e = tid; e < DD; e += blockDim.x) C[e] = A2[e];
        if (tid == 0) st->g = g;
        __syncthreads();
    }
    // _eigen: C = (C + C^T) / 2; eigh; d = sqrt(where(d2 < 0, eps, d2)); C = B diag(d^2) B^T
    for (int e = tid; e < DD; e += blockDim.x) {
        const int i = e / D, j = e % D;
        A2[e] = (C[i * D + j] + C[j * D + i]) / 2.0;
    }
    __syncthreads();
    for (int e = tid; e < DD; e += blockDim.x) C[e] = A2[e];
    __syncthreads();
    jacobi_eigen(D, C, B, d2, A, A2, V, V2, self_, oth, dlt, partner, rotated, &nrot);
    for (int i = tid; i < D; i += blockDim.x) d[i] = sqrt(d2[i] < 0 ? CMA_EPS : d2[i]);
    __syncthreads();
    for (int e = tid; e < DD; e += blockDim.x) {
        const int i = e / D, j = e % D;
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += (B[i * D + k] * (d[k] * d[k])) * B[j * D + k];
        st->C[e] = s;
        st->B[e] = B[e];
    }
    for (int e = tid; e < h.dmax * h.dmax; e += blockDim.x) {
        const int i = e / h.dmax, j = e % h.dmax;
        st->BD[e] = (i < D && j < D) ? B[i * D + j] * d[j] : 0.0;
    }
    for (int i = tid; i < D; i += blockDim.x) {
        st->d[i] = d[i];
        if (TELL) {
            st->mean[i] = mean[i];
            st->ps[i] = ps[i];
            st->pc[i] = pc[i];
        }
    }
    if (TELL && tid == 0) st->sigma = sig;
}

}  // namespace

// ------------------------------------------------------------------ the handle
struct alp_cma {
    alp_points *pts = nullptr;
    CmaHyper hy{};
    SamplerArgs sa{};
    ExpandArgs ex{};
    std::vector<uint64_t> seeds;  // K: start k's sampler seed
    bool lens_free = false, shared_pose = false;
    DeviceBuffer<> dev;           // one allocation: K states, weights, X, candidates, losses, order, y_k, w_io, told losses
    CmaState *st = nullptr;
    double *w = nullptr, *X = nullptr, *cand = nullptr, *loss = nullptr, *ys = nullptr, *wio = nullptr, *vals = nullptr;
    int *order = nullptr;
    bool pending = false;         // generations enqueued, alp_cma_wait not yet called
    bool have_last = false;       // a device generation has run (alp_cma_fetch_last)
    int64_t rows() const { return (int64_t)hy.K * hy.P; }
};

namespace alp {
void cma_points_gone(alp_cma_t *h) { h->pts = nullptr; }
}  // namespace alp

namespace {

// the state of start k (mean, sigma, C, p_sigma, pc, g; B and d cold) with its seed, for upload_states
void fill_state(const alp_cma *h, int k, CmaState *s, const double *mean, double sigma, const double *C, const double *ps, const double *pc,
                int64_t g) {
    const int D = h->hy.D;
    memset(s, 0, sizeof(*s));
    for (int i = 0; i < D; ++i) {
        s->mean[i] = mean[i];
        s->ps[i] = ps[i];
        s->pc[i] = pc[i];
        s->d[i] = 1.0;
        s->B[i * D + i] = 1.0;           // the eigendecomposition below starts cold (cma.py: set_state clears B and D)
    }
    for (int e = 0; e < D * D; ++e) s->C[e] = C[e];
    s->sigma = sigma;
    s->g = g;
    s->k0 = (unsigned)h->seeds[(size_t)k];
    s->k1 = (unsigned)(h->seeds[(size_t)k] >> 32);
}

// states k0 .. k0 + n - 1 from the host, then their eigendecompositions (n workgroups)
int upload_states(alp_cma *h, int k0, int n, const CmaState *s) {
    hipStream_t st = ctx().stream;
    ALP_HIP(hipMemcpyAsync(h->st + k0, s, (size_t)n * sizeof(CmaState), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(cma_tell_kernel<false>, dim3(n), dim3(TELL_THREADS), 0, st, h->hy, h->st + k0, (const double *)h->w,
                       (const double *)h->X, (const double *)nullptr, (const double *)nullptr, h->loss, h->order, h->ys, h->wio);
    ALP_HIP(hipGetLastError());
    ALP_HIP(hipStreamSynchronize(st));    // s (host) must outlive its copy
    return ALP_OK;
}

int usable(alp_cma *h, const char *what) {
    if (int rc = require_init()) return rc;
    if (!h) return fail(ALP_EINVAL, "%s: handle is NULL", what);
    if (h->pending) return fail(ALP_ESTATE, "%s: generations are enqueued; call alp_cma_wait first", what);
    return ALP_OK;
}

template <typename T, int DMAX>
void launch_generation(alp_cma *h, unsigned grid, hipStream_t st) {
    alp_points *p = h->pts;
    PoseRec<T> *recs = (PoseRec<T> *)p->cand_dev;
    if (h->lens_free)
        hipLaunchKernelGGL((cma_generation_kernel<T, DMAX, true>), dim3(grid), dim3(256), 0, st, h->sa, h->ex, (const CmaState *)h->st,
                           (long long)h->hy.P, (long long)h->rows(), h->X, h->cand, recs, (long long)p->cand_cap);
    else
        hipLaunchKernelGGL((cma_generation_kernel<T, DMAX, false>), dim3(grid), dim3(256), 0, st, h->sa, h->ex, (const CmaState *)h->st,
                           (long long)h->hy.P, (long long)h->rows(), h->X, h->cand, recs, (long long)p->cand_cap);
}

template <typename T>
void launch_generation_t(alp_cma *h, unsigned grid, hipStream_t st) {
    if (h->hy.dmax == 12) launch_generation<T, 12>(h, grid, st);
    else if (h->hy.dmax == 24) launch_generation<T, 24>(h, grid, st);
    else launch_generation<T, 32>(h, grid, st);
}

}  // namespace

extern "C" {

int alp_cma_create_starts(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                          const double *upper, int64_t P, int K, const double *weights, const double hyper[ALP_CMA_NHYPER],
                          int n_max_resampling, const uint64_t *seeds, alp_cma_t **out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(out, "out is NULL");
    *out = nullptr;
    ALP_REQUIRE(pts && tmpl && target_idx && lower && upper && weights && hyper && seeds, "NULL argument");
    ALP_REQUIRE(D >= 1 && D <= CMA_MAX_D, "D must be in [1, 32]");
    ALP_REQUIRE(P >= 1 && P <= CMA_MAX_P, "P must be in [1, 4096]");
    ALP_REQUIRE(K >= 1 && K <= CMA_MAX_STARTS, "K must be in [1, 1024]");
    ALP_REQUIRE((int64_t)K * P <= CMA_MAX_TOTAL, "K * P must be at most 65536");
    ALP_REQUIRE(n_max_resampling >= 0 && n_max_resampling <= (1 << 20), "n_max_resampling out of range");
    if (!pts->uo) return fail(ALP_ESTATE, "alp_cma_create: observed uv not set");
    for (int i = 0; i < D; ++i) {
        ALP_REQUIRE(target_idx[i] >= 0 && target_idx[i] < ALP_NPARAM, "target index out of range");
        ALP_REQUIRE(target_idx[i] != 21 && target_idx[i] != 22, "w and h cannot be targets (every candidate must share the image size)");
    }
    const int mu = (int)hyper[0];
    ALP_REQUIRE(mu >= 0 && mu <= P, "mu out of range");
    alp_cma *h = new alp_cma();
    h->pts = pts;
    const int dmax = D <= 12 ? 12 : (D <= 24 ? 24 : 32);
    h->hy = CmaHyper{D, (int)P, mu, dmax, K, hyper[1], hyper[2], hyper[3], hyper[4], hyper[5], hyper[6], hyper[7], hyper[8], hyper[9]};
    h->seeds.assign(seeds, seeds + K);
    memset(&h->sa, 0, sizeof(h->sa));
    for (int i = 0; i < D; ++i) {
        h->sa.lower[i] = 0.0;            // the normalised box of optimize.py: [0, 1]^D
        h->sa.upper[i] = 1.0;
    }
    h->sa.D = D;
    h->sa.n_max = n_max_resampling;
    h->sa.bounded = 1;                   // (the key comes from each start's state)
    memset(&h->ex, 0, sizeof(h->ex));
    for (int k = 0; k < ALP_NPARAM; ++k) h->ex.tmpl[k] = tmpl[k];
    for (int i = 0; i < D; ++i) {
        h->ex.idx[i] = target_idx[i];
        h->ex.lo[i] = lower[i];
        h->ex.hi[i] = upper[i];
    }
    memcpy(h->ex.origin, pts->origin, sizeof(h->ex.origin));
    // the kernel variant, once, by the rules enqueue_popeval applies to every population: lens-free when no target is a lens
    // coefficient k1..s4 and the template's are all 0; shared pose when every target is one of a1..s4 (the pose rows are then
    // the same for every candidate)
    bool lf = !getenv("ALP_POP_NO_LENS_FREE");
    for (int k = 9; k <= 20 && lf; ++k) lf = tmpl[k] == 0.0;
    for (int i = 0; i < D && lf; ++i) lf = !(target_idx[i] >= 9 && target_idx[i] <= 20);
    bool shared = P > 1 && !lf;
    for (int i = 0; i < D && shared; ++i) shared = target_idx[i] >= 7 && target_idx[i] <= 20;
    h->lens_free = lf;
    h->shared_pose = shared;
    const int64_t R = (int64_t)K * P;
    const size_t sz_state = round_up((int64_t)K * sizeof(CmaState), 256), sz_w = round_up(P * 8, 256), sz_p = round_up(R * 8, 256),
                 sz_pd = round_up(R * D * 8, 256), sz_cand = round_up(R * ALP_NPARAM * 8, 256), sz_ord = round_up(R * 4, 256);
    int rc = h->dev.reserve(sz_state + sz_w + 3 * sz_p + 2 * sz_pd + sz_cand + sz_ord);
    if (!rc) {
        char *q = (char *)h->dev;
        h->st = (CmaState *)q; q += sz_state;
        h->w = (double *)q; q += sz_w;
        h->loss = (double *)q; q += sz_p;
        h->wio = (double *)q; q += sz_p;
        h->vals = (double *)q; q += sz_p;
        h->X = (double *)q; q += sz_pd;
        h->ys = (double *)q; q += sz_pd;
        h->cand = (double *)q; q += sz_cand;
        h->order = (int *)q;
        if (hipMemcpy(h->w, weights, (size_t)P * 8, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ALP_EHIP, "alp_cma_create: weights upload failed");
    }
    if (!rc) rc = points_pop_reserve(pts, R);
    if (!rc) {                           // the state of a fresh cma.CMA(mean = 0.5, sigma = 1) per start: set_state replaces it
        std::vector<double> mean(D, 0.5), C((size_t)D * D, 0.0), zero(D, 0.0);
        for (int i = 0; i < D; ++i) C[(size_t)i * D + i] = 1.0;
        std::vector<CmaState> s((size_t)K);
        for (int k = 0; k < K; ++k) fill_state(h, k, &s[(size_t)k], mean.data(), 1.0, C.data(), zero.data(), zero.data(), 0);
        rc = upload_states(h, 0, K, s.data());
    }
    if (rc) {
        delete h;
        return rc;
    }
    pts->loops.push_back(h);
    *out = h;
    return ALP_OK;
}

int alp_cma_create(alp_points_t *pts, const double tmpl[ALP_NPARAM], const int32_t *target_idx, int D, const double *lower,
                   const double *upper, int64_t P, const double *weights, const double hyper[ALP_CMA_NHYPER], int n_max_resampling,
                   uint64_t seed, alp_cma_t **out) {
    return alp_cma_create_starts(pts, tmpl, target_idx, D, lower, upper, P, 1, weights, hyper, n_max_resampling, &seed, out);
}

int alp_cma_destroy(alp_cma_t *h) {
    if (!h) return ALP_OK;
    if (ctx().ready) hipStreamSynchronize(ctx().stream);
    if (h->pts) {
        h->pts->loop_pending = false;
        auto &v = h->pts->loops;
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] == h) {
                v.erase(v.begin() + (long)i);
                break;
            }
    }
    delete h;
    return ALP_OK;
}

int alp_cma_set_state_at(alp_cma_t *h, int k, const double *mean, double sigma, const double *C, const double *p_sigma, const double *pc,
                         int64_t generation) {
    if (int rc = usable(h, "alp_cma_set_state")) return rc;
    ALP_REQUIRE(k >= 0 && k < h->hy.K, "start index out of range");
    ALP_REQUIRE(mean && C && p_sigma && pc, "NULL argument");
    ALP_REQUIRE(sigma > 0, "sigma must be positive");
    ALP_REQUIRE(generation >= 0, "generation is negative");
    CmaState s;
    fill_state(h, k, &s, mean, sigma, C, p_sigma, pc, generation);
    return upload_states(h, k, 1, &s);
}

int alp_cma_set_state(alp_cma_t *h, const double *mean, double sigma, const double *C, const double *p_sigma, const double *pc,
                      int64_t generation) {
    return alp_cma_set_state_at(h, 0, mean, sigma, C, p_sigma, pc, generation);
}

int alp_cma_get_state_at(alp_cma_t *h, int k, double *mean, double *sigma, double *C, double *p_sigma, double *pc, int64_t *generation,
                         double *B, double *Dvec) {
    if (int rc = usable(h, "alp_cma_get_state")) return rc;
    ALP_REQUIRE(k >= 0 && k < h->hy.K, "start index out of range");
    CmaState s;
    ALP_HIP(hipMemcpyAsync(&s, h->st + k, sizeof(s), hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    const int D = h->hy.D;
    for (int i = 0; i < D; ++i) {
        if (mean) mean[i] = s.mean[i];
        if (p_sigma) p_sigma[i] = s.ps[i];
        if (pc) pc[i] = s.pc[i];
        if (Dvec) Dvec[i] = s.d[i];
    }
    for (int e = 0; e < D * D; ++e) {
        if (C) C[e] = s.C[e];
        if (B) B[e] = s.B[e];
    }
    if (sigma) *sigma = s.sigma;
    if (generation) *generation = s.g;
    return ALP_OK;
}

int alp_cma_get_state(alp_cma_t *h, double *mean, double *sigma, double *C, double *p_sigma, double *pc, int64_t *generation, double *B,
                      double *Dvec) {
    return alp_cma_get_state_at(h, 0, mean, sigma, C, p_sigma, pc, generation, B, Dvec);
}

int alp_cma_run(alp_cma_t *h, int64_t generations, int loss_kind, double f_scale) {
    if (int rc = usable(h, "alp_cma_run")) return rc;
    ALP_REQUIRE(generations >= 0, "generations is negative");
    ALP_REQUIRE(loss_kind == ALP_LOSS_MEAN_DIST || loss_kind == ALP_LOSS_HUBER, "unknown loss_kind");
    alp_points *p = h->pts;
    if (!p) return fail(ALP_ESTATE, "alp_cma_run: the point set of this device loop has been destroyed");
    if (p->pending_P > 0 || p->loop_pending)
        return fail(ALP_ESTATE, "alp_cma_run: the point set has an evaluation enqueued that has not been waited for");
    if (generations == 0) return ALP_OK;
    const int64_t R = h->rows();
    if (int rc = points_pop_reserve(p, R)) return rc;
    const unsigned grid = (unsigned)((R * 64 + 255) / 256);
    const bool batched = h->hy.K > 1;    // one start: the grid of alp_eval_population, as before multi-start
    hipStream_t st = ctx().stream;
    h->pending = true;                   // from the first launch on: a failure below still needs alp_cma_wait
    p->loop_pending = true;
    for (int64_t g = 0; g < generations; ++g) {
        if (p->precision == ALP_F64) launch_generation_t<double>(h, grid, st);
        else launch_generation_t<float>(h, grid, st);
        ALP_HIP(hipGetLastError());
        if (int rc = popeval_launch(p, R, loss_kind, f_scale, h->lens_free, h->shared_pose, batched, h->cand)) return rc;
        hipLaunchKernelGGL(cma_tell_kernel<true>, dim3(h->hy.K), dim3(TELL_THREADS), 0, st, h->hy, h->st, (const double *)h->w,
                           (const double *)h->X, (const double *)p->sums_dev, (const double *)nullptr, h->loss, h->order, h->ys, h->wio);
        ALP_HIP(hipGetLastError());
    }
    h->have_last = true;
    return ALP_OK;
}

int alp_cma_wait(alp_cma_t *h) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(h, "handle is NULL");
    if (!h->pending) return fail(ALP_ESTATE, "alp_cma_wait: nothing enqueued");
    h->pending = false;
    if (h->pts) h->pts->loop_pending = false;
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

int alp_cma_tell_host(alp_cma_t *h, const double *X, const double *losses, int32_t *order_out) {
    if (int rc = usable(h, "alp_cma_tell_host")) return rc;
    ALP_REQUIRE(X && losses, "NULL argument");
    const int64_t R = h->rows(), D = h->hy.D;
    hipStream_t st = ctx().stream;
    ALP_HIP(hipMemcpyAsync(h->X, X, (size_t)(R * D) * 8, hipMemcpyHostToDevice, st));
    ALP_HIP(hipMemcpyAsync(h->vals, losses, (size_t)R * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(cma_tell_kernel<true>, dim3(h->hy.K), dim3(TELL_THREADS), 0, st, h->hy, h->st, (const double *)h->w,
                       (const double *)h->X, (const double *)nullptr, (const double *)h->vals, h->loss, h->order, h->ys, h->wio);
    ALP_HIP(hipGetLastError());
    if (order_out) ALP_HIP(hipMemcpyAsync(order_out, h->order, (size_t)R * 4, hipMemcpyDeviceToHost, st));
    ALP_HIP(hipStreamSynchronize(st));
    h->have_last = false;                // X no longer holds a device generation
    return ALP_OK;
}

int alp_cma_fetch_last(alp_cma_t *h, double *X, double *cand, double *losses) {
    if (int rc = usable(h, "alp_cma_fetch_last")) return rc;
    if (!h->have_last) return fail(ALP_ESTATE, "alp_cma_fetch_last: no device generation has run");
    const int64_t R = h->rows(), D = h->hy.D;
    hipStream_t st = ctx().stream;
    if (X) ALP_HIP(hipMemcpyAsync(X, h->X, (size_t)(R * D) * 8, hipMemcpyDeviceToHost, st));
    if (cand) ALP_HIP(hipMemcpyAsync(cand, h->cand, (size_t)R * ALP_NPARAM * 8, hipMemcpyDeviceToHost, st));
    if (losses) ALP_HIP(hipMemcpyAsync(losses, h->loss, (size_t)R * 8, hipMemcpyDeviceToHost, st));
    ALP_HIP(hipStreamSynchronize(st));
    return ALP_OK;
}

}  // extern "C"
