// libalproj_hip.so -- the geometric match filter and the grid thinning that the reference's image_match runs between its matcher
// and set_gcp (src/alproj/gcp.py:507-544: _filter_geometric with outlier_filter="fundamental", then _filter_spatial).
//
// cv2's USAC (its random stream, PROSAC, SPRT, MAGSAC scoring) cannot be restated, so the filter is an algorithm of this project's
// own: hypothesise and verify outright.  H minimal samples of 8 matches -> H fundamental matrices by the normalised 8-point
// solve -> the inlier count of every one of them over all n matches -> the best one, refitted on its inliers while that strictly
// grows the count.  Everything is float64, and the unit is compiled with -ffp-contract=off: the error of a match under F is
// written in the order include/alproj_hip.h gives, so that numpy reproduces it bit for bit.
//
//   epi_pack_kernel       p1, p2 -> (x1, y1, x2, y2), 32 B per match
//   epi_norm_kernel       one workgroup: Hartley's normalisation of both images from all n points (centroid, mean distance sqrt 2)
//   epi_samples_kernel    a thread per hypothesis: 8 (the essential filter: 5, on a stream word of their own) distinct indices from the counter-based generator of alp_sampler.h keyed by
//                         (seed, hypothesis, attempt); a repeat is rejected and the next draw taken
//   epi_solve_kernel      a thread per hypothesis, 64 per workgroup.  The 8 x 9 matrix of the normalised sample lives in LDS, element
//                         e of lane l at e * 64 + l (72 doubles indexed by a pivot search would otherwise go to scratch); Gaussian
//                         elimination with complete pivoting, the null vector by back substitution, rank 2 by a one-sided Jacobi
//                         sweep over the three columns, T2^T F T1, unit Frobenius norm.  Rank below 8 or a non-finite F: NaN.
//   epi_solve5_kernel     the essential filter (reference gcp.py:200-252): a thread per sample of 5 matches, 64 per workgroup, Nister's
//                         five-point solver -> up to 10 essential matrices per sample as pixel-space matrices K^-T E K^-1, which
//                         everything below scores, chooses and refits like any other hypothesis (10 slots per sample, NaN = unused);
//                         the refit then projects onto the essential matrices (EpiState::essential).  Details at the kernel.
//   epi_score_kernel      a workgroup = 256 hypotheses (one per lane, F in registers) x one split of the match tiles.  A tile of
//                         512 matches is staged in LDS and every lane walks it: all lanes read the same address (a broadcast),
//                         the count stays in a register.  One division per error: max(s2 / a, s2 / b) = s2 / min(a, b) bit for
//                         bit, since a correctly rounded quotient is monotone in its divisor.
//   epi_merge_kernel      a thread per hypothesis: the sum of its partial counts over the splits (no atomics)
//   epi_choose_kernel     one workgroup: the highest count, the lowest index on a tie
//   epi_accum_kernel, epi_refit_kernel, epi_count_kernel, epi_decide_kernel
//                         one refit: the upper triangle of sum a a^T over the inliers of the current F (45 sums per lane, wave and
//                         workgroup reduction, fixed order), its smallest eigenvector by Jacobi rotations in one wave, rank 2,
//                         the count of the candidate, and the decision.  All of them read `stopped` from the state record and return
//                         at once when it is set: the host enqueues `refits` rounds and never looks.
//   epi_mask_kernel       mask and error of every match under one F
//   epi_select_kernel, epi_select_merge_kernel
//                         the LMedS filter: the rank-th smallest error of every hypothesis, exactly, without an H x n array: a
//                         radix select on the 64 bits of the error, the most significant 4-bit digit first, 16 passes.  The
//                         layout is the score kernel's; in every pass a lane forms its errors again and, for each one whose
//                         higher digits equal the prefix found so far, bumps one of 16 counters in LDS (counter d of lane l at
//                         d * 256 + l: a lane's own column, no bank conflict).  The merge adds the splits' counters in order
//                         (integers), finds the digit at which they reach the remaining rank and extends the prefix.
//   epi_lmeds_choose_kernel, epi_errs_kernel, epi_lmeds_eval_kernel
//                         the smallest value, the lowest index on a tie; the errors of one F (the chosen one, a refit's candidate)
//                         as an array; and one workgroup that selects the value of that array (8-bit digits, integer LDS
//                         atomics, 8 passes), forms the bound, counts the inliers and decides like epi_decide_kernel
//   thin_*_kernel         alp_grid_thin: atomic minima on (distance bits) and then on the index, per cell
#include "alp_sampler.h"

#include <climits>
#include <cmath>

namespace {

using namespace alp;

typedef unsigned long long u64;

struct EpiState {
    double T[6];                  // cx1, cy1, s1, cx2, cy2, s2: x' = (x - c) * s
    double Fcur[9], Fcand[9];
    long long info[EPI_INFO];
    int count, stopped, keep_all;
    int essential;                // T is K twice over (cx, cy, 1 / f) and a fitted matrix is projected onto the essential ones
    // the LMedS filter (alp_epipolar_lmeds / alp_essential_lmeds): a match is an inlier iff e <= bound2, which the value of the
    // current F sets, and `count` is the number of inliers at that bound
    int lmeds, rank;              // rank: 1-based, the order statistic that is a hypothesis' value
    double scale2, floor2;        // bound2 = max(scale2 * value, floor2)
    double value, bound2;         // of Fcur
    double stats[EPI_LMEDS_STATS];
};
static_assert(sizeof(EpiState) <= EPI_STATE_BYTES, "the state record outgrew its slot");

// info words of alp_epipolar_ransac
enum { I_CHOSEN = 0, I_CHOSEN_COUNT, I_FINAL_COUNT, I_REFITS_RUN, I_REFITS_KEPT, I_KEEP_ALL, I_HYP_TILE, I_MATCH_TILE, I_SPLITS,
       I_WORKGROUPS, I_BYTES, I_REDUCE_BLOCKS, I_REFIT_COUNT0 };
static_assert(I_REFIT_COUNT0 + EPI_MAX_REFITS <= EPI_INFO, "info too short");

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// the three quantities of the error expression, in the header's order
__device__ __forceinline__ void epi_terms(const double (&F)[9], double x1, double y1, double x2, double y2, double &ss, double &d2,
                                          double &d1) {
    const double l20 = (F[0] * x1 + F[1] * y1) + F[2];
    const double l21 = (F[3] * x1 + F[4] * y1) + F[5];
    const double l22 = (F[6] * x1 + F[7] * y1) + F[8];
    const double l10 = (F[0] * x2 + F[3] * y2) + F[6];
    const double l11 = (F[1] * x2 + F[4] * y2) + F[7];
    const double s = (x2 * l20 + y2 * l21) + l22;
    ss = s * s;
    d2 = l20 * l20 + l21 * l21;
    d1 = l10 * l10 + l11 * l11;
}

// e as written: the larger of the two quotients, NaN when either is
__device__ __forceinline__ double epi_error(const double (&F)[9], const double4 q) {
    double ss, d2, d1;
    epi_terms(F, q.x, q.y, q.z, q.w, ss, d2, d1);
    const double e2 = ss / d2, e1 = ss / d1;
    return e2 != e2 ? e2 : e1 != e1 ? e1 : e2 > e1 ? e2 : e1;
}

// e <= t2 with one division (the score kernel): the larger quotient is the one by the smaller divisor
__device__ __forceinline__ bool epi_inlier(const double (&F)[9], const double4 q, double t2) {
    double ss, d2, d1;
    epi_terms(F, q.x, q.y, q.z, q.w, ss, d2, d1);
    double dm = d1 < d2 ? d1 : d2;
    if (d1 != d1) dm = d1;
    return ss / dm <= t2;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of v over a workgroup of 256, the same value in every thread (buf: 4 doubles of LDS)
__device__ __forceinline__ double block_sum256(double v, double *buf) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    return (buf[0] + buf[1]) + (buf[2] + buf[3]);
}

__global__ __launch_bounds__(256) void epi_pack_kernel(const double2 *__restrict__ p1, const double2 *__restrict__ p2, int n,
                                                       double4 *__restrict__ pts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 a = p1[i], b = p2[i];
    pts[i] = make_double4(a.x, a.y, b.x, b.y);
}

__global__ __launch_bounds__(256) void epi_norm_kernel(const double4 *__restrict__ pts, int n, EpiState *__restrict__ st) {
    __shared__ double buf[4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256) {
        const double4 q = pts[i];
        s[0] += q.x, s[1] += q.y, s[2] += q.z, s[3] += q.w;
    }
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = block_sum256(s[k], buf) / (double)n;
    double m1 = 0.0, m2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double4 q = pts[i];
        const double ax = q.x - c[0], ay = q.y - c[1], bx = q.z - c[2], by = q.w - c[3];
        m1 += sqrt(ax * ax + ay * ay);
        m2 += sqrt(bx * bx + by * by);
    }
    m1 = block_sum256(m1, buf) / (double)n;
    m2 = block_sum256(m2, buf) / (double)n;
    if (threadIdx.x == 0) {
        st->T[0] = c[0], st->T[1] = c[1], st->T[2] = 1.4142135623730951 / m1;
        st->T[3] = c[2], st->T[4] = c[3], st->T[5] = 1.4142135623730951 / m2;
    }
}

constexpr int EPI_MAX_ATTEMPTS = 4096;
constexpr unsigned EPI_STREAM = 0x45504950u;      // the generator's third counter word: this unit's stream of 8-wide rows
constexpr unsigned EPI_STREAM5 = 0x45504935u;     // and the stream of the 5-wide rows: the 8-wide rows of a seed do not depend on it

template <int WIDTH, unsigned STREAM>
__global__ __launch_bounds__(256) void epi_samples_kernel(int n, int H, unsigned k0, unsigned k1, int *__restrict__ samples) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    int row[WIDTH];
#pragma unroll
    for (int i = 0; i < WIDTH; ++i) row[i] = -1;
    int filled = 0;
    auto offer = [&](int c) {
        bool dup = false;
#pragma unroll
        for (int i = 0; i < WIDTH; ++i) dup = dup || row[i] == c;
        if (!dup && filled < WIDTH) {
#pragma unroll
            for (int i = 0; i < WIDTH; ++i)
                if (i == filled) row[i] = c;
            ++filled;
        }
    };
    for (int attempt = 0; filled < WIDTH && attempt < EPI_MAX_ATTEMPTS; ++attempt) {
        unsigned w[4];
        philox4x32_10((unsigned)attempt, (unsigned)h, STREAM, 0u, k0, k1, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) offer((int)(((u64)w[j] * (u64)(unsigned)n) >> 32));
    }
    for (int c = 0; filled < WIDTH && c < n; ++c) offer(c);      // (never in practice: 16 384 draws without a full row)
#pragma unroll
    for (int i = 0; i < WIDTH; ++i) samples[(size_t)h * WIDTH + i] = row[i];
}

// m: a 3 x 3 matrix in normalised coordinates -> out: T2^T m T1 at unit Frobenius norm; NaN when that is not finite
__device__ void denorm_unit(const double (&m)[3][3], const double *__restrict__ T, double (&out)[9]) {
    // m T1, then T2^T (m T1)
    const double cx1 = T[0], cy1 = T[1], s1 = T[2], cx2 = T[3], cy2 = T[4], s2 = T[5];
    double a[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        a[r][0] = s1 * m[r][0];
        a[r][1] = s1 * m[r][1];
        a[r][2] = m[r][2] - s1 * (cx1 * m[r][0] + cy1 * m[r][1]);
    }
    double o[9], fro = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = s2 * a[0][c];
        o[3 + c] = s2 * a[1][c];
        o[6 + c] = a[2][c] - s2 * (cx2 * a[0][c] + cy2 * a[1][c]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) fro += o[k] * o[k];
    fro = sqrt(fro);
    const bool ok = fro > 0.0 && fro < INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = ok ? o[k] / fro : nan64();
}

// f: a 3 x 3 matrix in normalised coordinates, row-major -> out: its smallest singular value zeroed (essential: and the two
// others replaced by their mean), T2^T f T1, unit Frobenius norm; NaN when that is not finite
__device__ void rank2_denorm(const double (&f)[9], const double *__restrict__ T, bool essential, double (&out)[9]) {
    double g[3][3], v[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[r][c] = f[3 * r + c], v[r][c] = r == c ? 1.0 : 0.0;
    // one-sided Jacobi: rotate pairs of columns of g until they are orthogonal; g = U S, f = g v^T
    for (int sweep = 0; sweep < 16; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double alpha = (g[0][p] * g[0][p] + g[1][p] * g[1][p]) + g[2][p] * g[2][p];
            const double beta = (g[0][q] * g[0][q] + g[1][q] * g[1][q]) + g[2][q] * g[2][q];
            const double gamma = (g[0][p] * g[0][q] + g[1][p] * g[1][q]) + g[2][p] * g[2][q];
            if (gamma != 0.0 && fabs(gamma) > 1e-17 * sqrt(alpha * beta)) {
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double gp = g[r][p], gq = g[r][q], vp = v[r][p], vq = v[r][q];
                    g[r][p] = c * gp - s * gq, g[r][q] = s * gp + c * gq;
                    v[r][p] = c * vp - s * vq, v[r][q] = s * vp + c * vq;
                }
            }
        }
        if (!rotated) break;
    }
    double nrm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nrm[c] = (g[0][c] * g[0][c] + g[1][c] * g[1][c]) + g[2][c] * g[2][c];
    const int drop = nrm[0] <= nrm[1] ? (nrm[0] <= nrm[2] ? 0 : 2) : (nrm[1] <= nrm[2] ? 1 : 2);
    // the singular values are the column norms of g: (s, s, 0) with s their mean scales each kept column by s / its norm
    double scale[3] = {1.0, 1.0, 1.0};
    if (essential) {
        double sv[3], sum = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) sv[c] = sqrt(nrm[c]), sum += c == drop ? 0.0 : sv[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) scale[c] = (0.5 * sum) / sv[c];
    }
    double m[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) a += (j == drop ? 0.0 : g[r][j] * scale[j]) * v[c][j];
            m[r][c] = a;
        }
    denorm_unit(m, T, out);
}

constexpr double EPI_RANK_TOL = 1e-13;        // a pivot below this share of the first one: the sample's matrix has rank below 8

__global__ __launch_bounds__(EPI_SOLVE_BLOCK) void epi_solve_kernel(const double4 *__restrict__ pts, const int *__restrict__ samples, int H,
                                                                    const EpiState *__restrict__ st, double *__restrict__ Fout) {
    __shared__ double A_[72 * EPI_SOLVE_BLOCK];
    __shared__ double Y_[9 * EPI_SOLVE_BLOCK];
    __shared__ double X_[9 * EPI_SOLVE_BLOCK];
    const int lane = threadIdx.x;
    const int h = blockIdx.x * EPI_SOLVE_BLOCK + lane;
    if (h >= H) return;                 // no barrier below: a lane touches its own LDS column only
#define A(i, j) A_[((i) * 9 + (j)) * EPI_SOLVE_BLOCK + lane]
#define Y(j) Y_[(j) * EPI_SOLVE_BLOCK + lane]
#define X(j) X_[(j) * EPI_SOLVE_BLOCK + lane]
    double T[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) T[k] = st->T[k];
    for (int i = 0; i < EPI_SAMPLE; ++i) {
        const double4 q = pts[samples[(size_t)h * EPI_SAMPLE + i]];
        const double x1 = (q.x - T[0]) * T[2], y1 = (q.y - T[1]) * T[2], x2 = (q.z - T[3]) * T[5], y2 = (q.w - T[4]) * T[5];
        A(i, 0) = x2 * x1, A(i, 1) = x2 * y1, A(i, 2) = x2;
        A(i, 3) = y2 * x1, A(i, 4) = y2 * y1, A(i, 5) = y2;
        A(i, 6) = x1, A(i, 7) = y1, A(i, 8) = 1.0;
    }
    u64 perm = 0;                       // 4 bits per column: which unknown stands in column j
    for (int j = 0; j < 9; ++j) perm |= (u64)j << (4 * j);
    bool ok = true;
    double first = 0.0;
    for (int k = 0; k < 8; ++k) {
        int pi = k, pj = k;
        double pv = -1.0;
        for (int i = k; i < 8; ++i)
            for (int j = k; j < 9; ++j) {
                const double a = fabs(A(i, j));
                if (!(a <= pv)) pv = a, pi = i, pj = j;        // (a NaN entry becomes the pivot and fails the test below)
            }
        if (k == 0) first = pv;
        if (!(pv > first * EPI_RANK_TOL) || !(pv < INFINITY)) {
            ok = false;
            break;
        }
        if (pi != k)
            for (int j = k; j < 9; ++j) {
                const double t = A(k, j);
                A(k, j) = A(pi, j), A(pi, j) = t;
            }
        if (pj != k) {
            for (int i = 0; i < 8; ++i) {
                const double t = A(i, k);
                A(i, k) = A(i, pj), A(i, pj) = t;
            }
            const u64 a = (perm >> (4 * k)) & 15, b = (perm >> (4 * pj)) & 15;
            perm = (perm & ~((u64)15 << (4 * k)) & ~((u64)15 << (4 * pj))) | a << (4 * pj) | b << (4 * k);
        }
        const double piv = A(k, k);
        for (int i = k + 1; i < 8; ++i) {
            const double mlt = A(i, k) / piv;
            for (int j = k + 1; j < 9; ++j) A(i, j) -= mlt * A(k, j);
        }
    }
    double f[9], out[9];
    if (ok) {
        Y(8) = 1.0;
        for (int k = 7; k >= 0; --k) {
            double s = 0.0;
            for (int j = k + 1; j < 9; ++j) s += A(k, j) * Y(j);
            Y(k) = -s / A(k, k);
        }
        for (int j = 0; j < 9; ++j) X((int)((perm >> (4 * j)) & 15)) = Y(j);
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = X(k);
        rank2_denorm(f, T, false, out);
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = nan64();
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Fout[(size_t)h * 9 + k] = out[k];
#undef A
#undef Y
#undef X
}

// ------------------------------------------------------------------ the five-point solver
// Nister's formulation with Stewenius' Gauss-Jordan step.  The unknowns are (x, y, z) of E = x N0 + y N1 + z N2 + N3 over the
// null space of the sample's 5 x 9 matrix; the ten cubics det E = 0 and 2 E E^T E - tr(E E^T) E = 0 are rows over 20 monomials
// in this column order, the first ten of which are eliminated:
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
// Polynomials of degree 1 are held over (x, y, z, 1), of degree 2 over (xx xy xz x yy yz y zz z 1); SOLVE5_IDX2[i * 4 + j] is the
// place of the product of two degree-1 terms, SOLVE5_IDX3[m * 4 + j] the column of a degree-2 term times a degree-1 term.  Every
// loop over them is unrolled, so the indices are constants and the polynomials stay in registers.
__device__ constexpr int SOLVE5_IDX2[16] = {0, 1, 2, 3, 1, 4, 5, 6, 2, 5, 7, 8, 3, 6, 8, 9};
__device__ constexpr int SOLVE5_IDX3[40] = {0, 2, 4,  5,  2, 3,  8,  9,  4,  8,  10, 11, 5,  9,  11, 12, 3,  1,  6,  7,
                                            8, 6, 13, 14, 9, 7,  14, 15, 10, 13, 16, 17, 11, 14, 17, 18, 12, 15, 18, 19};

// c += sign * a * b: degree 1 times degree 1
__device__ __forceinline__ void poly_mul11(const double (&a)[4], const double (&b)[4], double sign, double (&c)[10]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c[SOLVE5_IDX2[i * 4 + j]] += sign * (a[i] * b[j]);
}
// r += a * b: degree 2 times degree 1
__device__ __forceinline__ void poly_mul21(const double (&a)[10], const double (&b)[4], double (&r)[20]) {
#pragma unroll
    for (int m = 0; m < 10; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) r[SOLVE5_IDX3[m * 4 + j]] += a[m] * b[j];
}

// g: det E and the nine entries of 2 E E^T E - tr(E E^T) E
__device__ void ess_constraints(const double (&E)[9], double (&g)[10]) {
    double S[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
    const double tr = (S[0][0] + S[1][1]) + S[2][2];
    g[0] = (E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6])) + E[2] * (E[3] * E[7] - E[4] * E[6]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            g[1 + 3 * i + j] = 2.0 * ((S[i][0] * E[j] + S[i][1] * E[3 + j]) + S[i][2] * E[6 + j]) - tr * E[3 * i + j];
}

// d: the derivative of ess_constraints at E in the direction N
__device__ void ess_derivative(const double (&E)[9], const double (&N)[9], double (&d)[10]) {
    double S[3][3], dS[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            S[i][j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
            dS[i][j] = ((N[3 * i] * E[3 * j] + N[3 * i + 1] * E[3 * j + 1]) + N[3 * i + 2] * E[3 * j + 2]) +
                       ((E[3 * i] * N[3 * j] + E[3 * i + 1] * N[3 * j + 1]) + E[3 * i + 2] * N[3 * j + 2]);
        }
    const double tr = (S[0][0] + S[1][1]) + S[2][2], dtr = (dS[0][0] + dS[1][1]) + dS[2][2];
    d[0] = ((N[0] * (E[4] * E[8] - E[5] * E[7]) - N[1] * (E[3] * E[8] - E[5] * E[6])) + N[2] * (E[3] * E[7] - E[4] * E[6])) +
           ((N[3] * (E[2] * E[7] - E[1] * E[8]) - N[4] * (E[2] * E[6] - E[0] * E[8])) + N[5] * (E[1] * E[6] - E[0] * E[7])) +
           ((N[6] * (E[1] * E[5] - E[2] * E[4]) - N[7] * (E[0] * E[5] - E[2] * E[3])) + N[8] * (E[0] * E[4] - E[1] * E[3]));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d[1 + 3 * i + j] = 2.0 * (((dS[i][0] * E[j] + dS[i][1] * E[3 + j]) + dS[i][2] * E[6 + j]) +
                                      ((S[i][0] * N[j] + S[i][1] * N[3 + j]) + S[i][2] * N[6 + j])) -
                               (dtr * E[3 * i + j] + tr * N[3 * i + j]);
}

constexpr int SOLVE5_POLISH = 3;              // Gauss-Newton steps on the ten cubics at every solution
constexpr double SOLVE5_POLISH_TOL = 5e-14;   // |cubics| of E at unit norm above this after the steps: they did not converge, no solution
constexpr int SOLVE5_BISECTIONS = 200;        // (an interval of doubles is exhausted long before)

// A thread per sample, 64 per workgroup.  What is indexed by a pivot search or a loop counter lives in LDS, word w of lane l at
// w * 64 + l: first the 5 x 9 matrix of the sample and its null vectors, then the 10 x 20 matrix of the cubics, then the
// derivatives of the degree-10 polynomial and the roots of two neighbouring ones.  200 words a lane: 100 KB, one workgroup on a
// CU.  The polynomials in (x, y, z) that the cubics are expanded from are indexed by constants and stay in registers.
__global__ __launch_bounds__(EPI_SOLVE_BLOCK) void epi_solve5_kernel(const double4 *__restrict__ pts, const int *__restrict__ samples, int H,
                                                                     const EpiState *__restrict__ st, double *__restrict__ Fout,
                                                                     int *__restrict__ nsol) {
    __shared__ double W_[200 * EPI_SOLVE_BLOCK];
    const int lane = threadIdx.x;
    const int h = blockIdx.x * EPI_SOLVE_BLOCK + lane;
    if (h >= H) return;                 // no barrier below: a lane touches its own LDS column only
#define W(i) W_[(i) * EPI_SOLVE_BLOCK + lane]
#define A(i, j) W((i) * 9 + (j))
#define Y(j) W(45 + (j))
#define NV(c, j) W(54 + (c) * 9 + (j))
#define M(i, j) W((i) * 20 + (j))
    double T[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) T[k] = st->T[k];
    double *const out = Fout + (size_t)h * 90;
    for (int k = 0; k < 90; ++k) out[k] = nan64();
    nsol[h] = 0;

    // ---- the null space of the 5 x 9 matrix: elimination with complete pivoting, as epi_solve_kernel does it
    for (int i = 0; i < 5; ++i) {
        const double4 q = pts[samples[(size_t)h * 5 + i]];
        const double x1 = (q.x - T[0]) * T[2], y1 = (q.y - T[1]) * T[2], x2 = (q.z - T[3]) * T[5], y2 = (q.w - T[4]) * T[5];
        A(i, 0) = x2 * x1, A(i, 1) = x2 * y1, A(i, 2) = x2;
        A(i, 3) = y2 * x1, A(i, 4) = y2 * y1, A(i, 5) = y2;
        A(i, 6) = x1, A(i, 7) = y1, A(i, 8) = 1.0;
    }
    u64 perm = 0;                       // 4 bits per column: which unknown stands in column j
    for (int j = 0; j < 9; ++j) perm |= (u64)j << (4 * j);
    double first = 0.0;
    for (int k = 0; k < 5; ++k) {
        int pi = k, pj = k;
        double pv = -1.0;
        for (int i = k; i < 5; ++i)
            for (int j = k; j < 9; ++j) {
                const double a = fabs(A(i, j));
                if (!(a <= pv)) pv = a, pi = i, pj = j;
            }
        if (k == 0) first = pv;
        if (!(pv > first * EPI_RANK_TOL) || !(pv < INFINITY)) return;
        if (pi != k)
            for (int j = k; j < 9; ++j) {
                const double t = A(k, j);
                A(k, j) = A(pi, j), A(pi, j) = t;
            }
        if (pj != k) {
            for (int i = 0; i < 5; ++i) {
                const double t = A(i, k);
                A(i, k) = A(i, pj), A(i, pj) = t;
            }
            const u64 a = (perm >> (4 * k)) & 15, b = (perm >> (4 * pj)) & 15;
            perm = (perm & ~((u64)15 << (4 * k)) & ~((u64)15 << (4 * pj))) | a << (4 * pj) | b << (4 * k);
        }
        const double piv = A(k, k);
        for (int i = k + 1; i < 5; ++i) {
            const double mlt = A(i, k) / piv;
            for (int j = k + 1; j < 9; ++j) A(i, j) -= mlt * A(k, j);
        }
    }
    // null vector c: 1 at free column 5 + c, 0 at the other three, the rest by back substitution
    for (int c = 0; c < 4; ++c) {
        for (int j = 5; j < 9; ++j) Y(j) = j == 5 + c ? 1.0 : 0.0;
        for (int k = 4; k >= 0; --k) {
            double s = 0.0;
            for (int j = k + 1; j < 9; ++j) s += A(k, j) * Y(j);
            Y(k) = -s / A(k, k);
        }
        for (int j = 0; j < 9; ++j) NV(c, (int)((perm >> (4 * j)) & 15)) = Y(j);
    }
    double Ep[9][4];                    // entry k of E as a polynomial over (x, y, z, 1)
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) Ep[k][c] = NV(c, k);

    // ---- the ten cubics, each expanded in registers and stored as a row of M (from here on A, Y and NV are dead)
    {
        double L[6][10];                // 2 E E^T - tr(E E^T) I, the upper triangle: 00 01 02 11 12 22
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int i = t < 3 ? 0 : t < 5 ? 1 : 2, j = t < 3 ? t : t < 5 ? t - 2 : 2;
#pragma unroll
            for (int m = 0; m < 10; ++m) L[t][m] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) poly_mul11(Ep[3 * i + k], Ep[3 * j + k], 2.0, L[t]);
        }
#pragma unroll
        for (int m = 0; m < 10; ++m) {
            const double tr = 0.5 * ((L[0][m] + L[3][m]) + L[5][m]);
            L[0][m] -= tr, L[3][m] -= tr, L[5][m] -= tr;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double r[20];
#pragma unroll
                for (int m = 0; m < 20; ++m) r[m] = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int lo = i < k ? i : k, hi = i < k ? k : i;
                    poly_mul21(L[lo == 0 ? hi : lo == 1 ? 2 + hi : 5], Ep[3 * k + j], r);
                }
#pragma unroll
                for (int m = 0; m < 20; ++m) M(1 + 3 * i + j, m) = r[m];
            }
    }
    {
        double r[20];
#pragma unroll
        for (int m = 0; m < 20; ++m) r[m] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {   // the cofactor of E[2][j] times E[2][j]
            const int a = j == 0 ? 1 : 0, b = j == 2 ? 1 : 2;
            double c[10];
#pragma unroll
            for (int m = 0; m < 10; ++m) c[m] = 0.0;
            poly_mul11(Ep[a], Ep[3 + b], j == 1 ? -1.0 : 1.0, c);
            poly_mul11(Ep[b], Ep[3 + a], j == 1 ? 1.0 : -1.0, c);
            poly_mul21(c, Ep[6 + j], r);
        }
#pragma unroll
        for (int m = 0; m < 20; ++m) M(0, m) = r[m];
    }

    // ---- Gauss-Jordan on the first ten columns, partial pivoting; rows 0..3 are not needed above their pivots
    for (int k = 0; k < 10; ++k) {
        int pi = k;
        double pv = -1.0;
        for (int i = k; i < 10; ++i) {
            const double a = fabs(M(i, k));
            if (!(a <= pv)) pv = a, pi = i;
        }
        if (!(pv > 0.0) || !(pv < INFINITY)) return;
        if (pi != k)
            for (int j = k; j < 20; ++j) {
                const double t = M(k, j);
                M(k, j) = M(pi, j), M(pi, j) = t;
            }
        const double piv = M(k, k);
        for (int j = k + 1; j < 20; ++j) M(k, j) /= piv;
        for (int i = 0; i < 10; ++i) {
            if (i == k || (i < k && i < 4)) continue;
            const double mlt = M(i, k);
            for (int j = k + 1; j < 20; ++j) M(i, j) -= mlt * M(k, j);
        }
    }
    // ---- B(z) (x, y, 1)^T = 0: row(x^2 z) - z row(x^2), row(y^2 z) - z row(y^2), row(xyz) - z row(xy); lowest power first
    double bx[3][4], by[3][4], bc[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double e[10], f[10];
#pragma unroll
        for (int t = 0; t < 10; ++t) e[t] = M(4 + 2 * r, 10 + t), f[t] = M(5 + 2 * r, 10 + t);
        bx[r][0] = e[2], bx[r][1] = e[1] - f[2], bx[r][2] = e[0] - f[1], bx[r][3] = -f[0];
        by[r][0] = e[5], by[r][1] = e[4] - f[5], by[r][2] = e[3] - f[4], by[r][3] = -f[3];
        bc[r][0] = e[9], bc[r][1] = e[8] - f[9], bc[r][2] = e[7] - f[8], bc[r][3] = e[6] - f[7], bc[r][4] = -f[6];
    }
    // p = det B = (bx0 by1 - by0 bx1) bc2 + (by0 bc1 - bc0 by1) bx2 + (bc0 bx1 - bx0 bc1) by2
    double p[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) p[k] = 0.0;
    {
        double m6[7], m7[8], n7[8];
#pragma unroll
        for (int k = 0; k < 7; ++k) m6[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) m7[k] = n7[k] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) m6[i + j] += bx[0][i] * by[1][j] - by[0][i] * bx[1][j];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                m7[i + j] += by[0][i] * bc[1][j] - bc[0][j] * by[1][i];
                n7[i + j] += bc[0][j] * bx[1][i] - bx[0][i] * bc[1][j];
            }
        }
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) p[i + j] += m6[i] * bc[2][j];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) p[i + j] += m7[i] * bx[2][j] + n7[i] * by[2][j];
    }

    // ---- every real root of p.  D(k, .) is the k-th derivative; between two neighbouring roots of D(k + 1) the polynomial D(k)
    // is monotone, so a change of sign there is one root and bisection finds it.  Cauchy's bound holds all roots of p, and
    // with them those of every derivative.
#define D(k, j) W((k) * 11 + (j))       // 0..109 (M is dead)
#define R(s, j) W(110 + (s) * 12 + (j)) // two root lists of at most 10
    double bound = 0.0;
    bool finite = true;                 // (fmax passes over a NaN, so the coefficients are tested themselves)
#pragma unroll
    for (int j = 0; j < 11; ++j) finite = finite && fabs(p[j]) < INFINITY;
#pragma unroll
    for (int j = 0; j < 10; ++j) bound = fmax(bound, fabs(p[j] / p[10]));
    bound += 1.0;
    if (!finite || !(bound < INFINITY)) return;       // a non-finite coefficient or a vanishing leading one
#pragma unroll
    for (int j = 0; j < 11; ++j) D(0, j) = p[j];
    for (int k = 1; k < 10; ++k)
        for (int j = 0; j <= 10 - k; ++j) D(k, j) = D(k - 1, j + 1) * (double)(j + 1);
    int nprev = 0, cur = 0;
    for (int deg = 1; deg <= 10; ++deg) {
        const int k = 10 - deg, prev = cur ^ 1;
        auto eval = [&](double z) {
            double a = D(k, deg);
            for (int j = deg - 1; j >= 0; --j) a = a * z + D(k, j);
            return a;
        };
        int nr = 0;
        double lo = -bound, flo = eval(lo);
        for (int s = 0; s <= nprev; ++s) {
            const double hi = s < nprev ? R(prev, s) : bound, fhi = eval(hi);
            if (fhi == 0.0) {
                if (nr < 10) R(cur, nr) = hi, ++nr;
            } else if (flo != 0.0 && (flo < 0.0) != (fhi < 0.0)) {
                double a = lo, b = hi, mid = 0.5 * (lo + hi);
                for (int it = 0; it < SOLVE5_BISECTIONS; ++it) {
                    mid = 0.5 * (a + b);
                    if (mid == a || mid == b) break;
                    const double fm = eval(mid);
                    if (fm == 0.0) break;
                    if ((fm < 0.0) == (flo < 0.0)) a = mid;
                    else b = mid;
                }
                if (nr < 10) R(cur, nr) = mid, ++nr;
            }
            lo = hi, flo = fhi;
        }
        nprev = nr, cur = prev;
    }
    const int roots = cur ^ 1;          // the list written last

    // ---- back substitution, Gauss-Newton steps on the ten cubics, K^-T E K^-1
    int found = 0;
    bool bad = false;
    for (int s = 0; s < nprev; ++s) {
        const double z = R(roots, s);
        double b[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            b[r][0] = ((bx[r][3] * z + bx[r][2]) * z + bx[r][1]) * z + bx[r][0];
            b[r][1] = ((by[r][3] * z + by[r][2]) * z + by[r][1]) * z + by[r][0];
            b[r][2] = (((bc[r][4] * z + bc[r][3]) * z + bc[r][2]) * z + bc[r][1]) * z + bc[r][0];
        }
        // (x, y, 1) is the cross product of two rows of B(z): of the three, the one with the largest third component
        double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int r0 = t == 2 ? 1 : 0, r1 = t == 0 ? 1 : 2;
            const double c0 = b[r0][1] * b[r1][2] - b[r0][2] * b[r1][1], c1 = b[r0][2] * b[r1][0] - b[r0][0] * b[r1][2],
                         c2 = b[r0][0] * b[r1][1] - b[r0][1] * b[r1][0];
            if (t == 0 || fabs(c2) > fabs(v[2])) v[0] = c0, v[1] = c1, v[2] = c2;
        }
        double u[3] = {v[0] / v[2], v[1] / v[2], z}, E[9], g[10];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = ((u[0] * Ep[k][0] + u[1] * Ep[k][1]) + u[2] * Ep[k][2]) + Ep[k][3];
        ess_constraints(E, g);
        double gg = 0.0;
#pragma unroll
        for (int k = 0; k < 10; ++k) gg += g[k] * g[k];
        for (int it = 0; it < SOLVE5_POLISH; ++it) {
            double J[3][10], N[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < 9; ++k) N[k] = Ep[k][c];
                ess_derivative(E, N, J[c]);
            }
            double a[3][3], rhs[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                rhs[r] = 0.0;
#pragma unroll
                for (int k = 0; k < 10; ++k) rhs[r] += J[r][k] * g[k];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    a[r][c] = 0.0;
#pragma unroll
                    for (int k = 0; k < 10; ++k) a[r][c] += J[r][k] * J[c][k];
                }
            }
            const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2],
                         c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
            const double det = (a[0][0] * c00 + a[0][1] * c01) + a[0][2] * c02;
            const double d0 = ((c00 * rhs[0] + (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * rhs[1]) + (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * rhs[2]) / det;
            const double d1 = ((c01 * rhs[0] + (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * rhs[1]) + (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * rhs[2]) / det;
            const double d2 = ((c02 * rhs[0] + (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * rhs[1]) + (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * rhs[2]) / det;
            const double w[3] = {u[0] - d0, u[1] - d1, u[2] - d2};
            double E2[9], g2[10], gg2 = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) E2[k] = ((w[0] * Ep[k][0] + w[1] * Ep[k][1]) + w[2] * Ep[k][2]) + Ep[k][3];
            ess_constraints(E2, g2);
#pragma unroll
            for (int k = 0; k < 10; ++k) gg2 += g2[k] * g2[k];
            if (!(gg2 < gg)) break;     // no better (or not finite): the step is not taken
            gg = gg2;
#pragma unroll
            for (int k = 0; k < 3; ++k) u[k] = w[k];
#pragma unroll
            for (int k = 0; k < 9; ++k) E[k] = E2[k];
#pragma unroll
            for (int k = 0; k < 10; ++k) g[k] = g2[k];
        }
        double nn = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) nn += E[k] * E[k];
        // the cubics are homogeneous of degree 3 in E: gg / nn^3 is their squared norm at unit E.  What the steps did not bring
        // onto them (a start too far off, a Jacobian without rank) is no essential matrix and no solution.
        if (!(gg <= (SOLVE5_POLISH_TOL * SOLVE5_POLISH_TOL) * ((nn * nn) * nn))) continue;
        const double m[3][3] = {{E[0], E[1], E[2]}, {E[3], E[4], E[5]}, {E[6], E[7], E[8]}};
        double f[9];
        denorm_unit(m, T, f);
        bad = bad || f[0] != f[0];
#pragma unroll
        for (int k = 0; k < 9; ++k) out[found * 9 + k] = f[k];
        ++found;
    }
    if (bad) {                          // a non-finite solution: the sample gives none
        for (int k = 0; k < 90; ++k) out[k] = nan64();
        found = 0;
    }
    nsol[h] = found;
#undef W
#undef A
#undef Y
#undef NV
#undef M
#undef D
#undef R
}

// the essential filter's state: K for both images in place of Hartley's normalisation
__global__ void epi_essential_kernel(double f, double cx, double cy, EpiState *__restrict__ st) {
    if (threadIdx.x != 0) return;
    st->T[0] = st->T[3] = cx, st->T[1] = st->T[4] = cy, st->T[2] = st->T[5] = 1.0 / f;
    st->essential = 1;
}

__global__ __launch_bounds__(EPI_HYP_TILE) void epi_score_kernel(const double4 *__restrict__ pts, int n, const double *__restrict__ F, int H,
                                                                 double t2, int splits, long long match_tiles, long long h_pad,
                                                                 int *__restrict__ partial) {
    __shared__ double4 tile[EPI_MATCH_TILE];
    const long long htile = blockIdx.x / (unsigned)splits;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const long long h = htile * EPI_HYP_TILE + threadIdx.x;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = h < H ? F[(size_t)h * 9 + k] : nan64();
    int64_t tb, te;
    match_split_range(match_tiles, splits, split, &tb, &te);
    int count = 0;
    for (long long t = tb; t < te; ++t) {
        const int base = (int)(t * EPI_MATCH_TILE);
        const int cnt = n - base < EPI_MATCH_TILE ? n - base : EPI_MATCH_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += EPI_HYP_TILE) tile[i] = pts[base + i];
        __syncthreads();
#pragma unroll 4
        for (int m = 0; m < cnt; ++m) count += epi_inlier(f, tile[m], t2) ? 1 : 0;
    }
    partial[(size_t)split * h_pad + h] = count;
}

__global__ __launch_bounds__(256) void epi_merge_kernel(const int *__restrict__ partial, int splits, long long h_pad, int H,
                                                        int *__restrict__ counts) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    int c = 0;
    for (int s = 0; s < splits; ++s) c += partial[(size_t)s * h_pad + h];
    counts[h] = c;
}

// the highest count, the lowest index on a tie: the largest key count << 32 | ~index
// min_count: the size of a minimal sample; a best count below it keeps every match
__global__ __launch_bounds__(256) void epi_choose_kernel(const int *__restrict__ counts, int H, const double *__restrict__ F, int min_count,
                                                         EpiState *__restrict__ st) {
    __shared__ u64 best[4];
    u64 key = 0;
    for (int h = threadIdx.x; h < H; h += 256) {
        const u64 k = (u64)(unsigned)counts[h] << 32 | (u64)(0xffffffffu - (unsigned)h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), o, 64);
        const u64 k = (u64)hi << 32 | lo;
        key = k > key ? k : key;
    }
    if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) key = best[w] > key ? best[w] : key;
        const int idx = (int)(0xffffffffu - (unsigned)key), count = (int)(key >> 32);
        for (int k = 0; k < 9; ++k) st->Fcur[k] = F[(size_t)idx * 9 + k], st->Fcand[k] = nan64();
        for (int k = 0; k < EPI_INFO; ++k) st->info[k] = 0;
        for (int k = 0; k < EPI_MAX_REFITS; ++k) st->info[I_REFIT_COUNT0 + k] = -1;
        st->count = count;
        st->keep_all = st->stopped = count < min_count ? 1 : 0;
        st->info[I_CHOSEN] = idx, st->info[I_CHOSEN_COUNT] = st->info[I_FINAL_COUNT] = count, st->info[I_KEEP_ALL] = st->keep_all;
    }
}

__global__ __launch_bounds__(EPI_REDUCE_BLOCK) void epi_accum_kernel(const double4 *__restrict__ pts, int n, double t2,
                                                                     const EpiState *__restrict__ st, double *__restrict__ sym) {
    __shared__ double red[4 * EPI_SYM];
    if (st->stopped) return;
    if (st->lmeds) t2 = st->bound2;
    double f[9], T[6], acc[EPI_SYM];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = st->Fcur[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) T[k] = st->T[k];
#pragma unroll
    for (int k = 0; k < EPI_SYM; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * EPI_REDUCE_BLOCK + threadIdx.x; i < n; i += gridDim.x * EPI_REDUCE_BLOCK) {
        const double4 q = pts[i];
        if (!(epi_error(f, q) <= t2)) continue;
        const double x1 = (q.x - T[0]) * T[2], y1 = (q.y - T[1]) * T[2], x2 = (q.z - T[3]) * T[5], y2 = (q.w - T[4]) * T[5];
        const double a[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
        int k = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int c = r; c < 9; ++c) acc[k++] += a[r] * a[c];
    }
#pragma unroll
    for (int k = 0; k < EPI_SYM; ++k) {
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * EPI_SYM + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < EPI_SYM)
        sym[(size_t)blockIdx.x * EPI_SYM + threadIdx.x] =
            (red[threadIdx.x] + red[EPI_SYM + threadIdx.x]) + (red[2 * EPI_SYM + threadIdx.x] + red[3 * EPI_SYM + threadIdx.x]);
}

// one wave: the 45 sums over the workgroups of epi_accum_kernel in order, then the eigenvector of the smallest eigenvalue of the
// 9 x 9 matrix by Jacobi rotations, four disjoint pairs at a time (matrix and vectors in LDS: they are indexed by the rotation's
// pair), and on lane 0 rank 2 and T2^T f T1
__global__ __launch_bounds__(64) void epi_refit_kernel(const double *__restrict__ sym, int blocks, EpiState *__restrict__ st) {
    __shared__ double S[EPI_SYM], M[81], V[81];
    if (st->stopped) return;
    if (threadIdx.x < EPI_SYM) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += sym[(size_t)b * EPI_SYM + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    const int i = threadIdx.x;          // lanes 0..8 own index i of every rotation; all lanes walk the pairs together
    for (int e = i; e < 81; e += 64) {
        const int r = e / 9, c = e % 9, lo_rc = r < c ? r : c, hi_rc = r < c ? c : r;
        M[e] = S[lo_rc * 9 - lo_rc * (lo_rc - 1) / 2 + (hi_rc - lo_rc)];
        V[e] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    // round-robin order: 9 rounds of 4 disjoint pairs cover the 36 pairs once (the circle method over 9 indices and a bye); the 4
    // rotations of a round touch different rows and columns, so M <- J^T M J is their columns, a barrier, their rows.  Lane
    // 9 k + e turns element e of pair k.
    const int pair = i / 9, e = i % 9;
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int round = 0; round < 9; ++round) {
            const int a = (round + pair + 1) % 9, b = (round + 8 - pair) % 9;
            const int p = a < b ? a : b, q = a < b ? b : a;
            bool rot = false;
            double c = 1.0, s = 0.0;
            if (pair < 4) {
                const double apq = M[p * 9 + q], app = M[p * 9 + p], aqq = M[q * 9 + q];
                rot = apq != 0.0 && fabs(apq) > 1e-17 * sqrt(fabs(app) * fabs(aqq));
                if (rot) {
                    const double zeta = (aqq - app) / (2.0 * apq);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                }
            }
            rotated = rotated || __any(rot);           // (the workgroup is one wave)
            __syncthreads();
            if (rot) {                                 // columns p, q of M and of V
                const double mp = M[e * 9 + p], mq = M[e * 9 + q], vp = V[e * 9 + p], vq = V[e * 9 + q];
                M[e * 9 + p] = c * mp - s * mq, M[e * 9 + q] = s * mp + c * mq;
                V[e * 9 + p] = c * vp - s * vq, V[e * 9 + q] = s * vp + c * vq;
            }
            __syncthreads();
            if (rot) {                                 // rows p, q
                const double mp = M[p * 9 + e], mq = M[q * 9 + e];
                M[p * 9 + e] = c * mp - s * mq, M[q * 9 + e] = s * mp + c * mq;
            }
            __syncthreads();
            if (rot && e == 0) M[p * 9 + q] = M[q * 9 + p] = 0.0;
            __syncthreads();
        }
        if (!rotated) break;
    }
    if (i != 0) return;
    int lo = 0;
    for (int i = 1; i < 9; ++i)
        if (M[i * 9 + i] < M[lo * 9 + lo]) lo = i;
    double f[9], out[9], T[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = V[i * 9 + lo];
#pragma unroll
    for (int i = 0; i < 6; ++i) T[i] = st->T[i];
    rank2_denorm(f, T, st->essential != 0, out);
#pragma unroll
    for (int i = 0; i < 9; ++i) st->Fcand[i] = out[i];
}

__global__ __launch_bounds__(EPI_REDUCE_BLOCK) void epi_count_kernel(const double4 *__restrict__ pts, int n, double t2,
                                                                     const EpiState *__restrict__ st, int *__restrict__ cpart) {
    __shared__ int red[4];
    if (st->stopped) return;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = st->Fcand[k];
    int c = 0;
    for (int i = blockIdx.x * EPI_REDUCE_BLOCK + threadIdx.x; i < n; i += gridDim.x * EPI_REDUCE_BLOCK)
        c += epi_error(f, pts[i]) <= t2 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void epi_decide_kernel(const int *__restrict__ cpart, int blocks, int round, EpiState *__restrict__ st) {
    if (threadIdx.x != 0 || st->stopped) return;
    int c = 0;
    for (int b = 0; b < blocks; ++b) c += cpart[b];
    st->info[I_REFIT_COUNT0 + round] = c;
    st->info[I_REFITS_RUN] = round + 1;
    if (c > st->count) {
        for (int k = 0; k < 9; ++k) st->Fcur[k] = st->Fcand[k];
        st->count = c;
        st->info[I_FINAL_COUNT] = c;
        st->info[I_REFITS_KEPT] += 1;
    } else {
        st->stopped = 1;
    }
}

// F: 9 doubles on the device; keep_all: NULL, or a flag on the device that turns every mask entry into 1; bound2: NULL, or the
// squared bound on the device that replaces t2 (the LMedS filter)
__global__ __launch_bounds__(256) void epi_mask_kernel(const double4 *__restrict__ pts, int n, const double *__restrict__ F, double t2,
                                                       const int *__restrict__ keep_all, const double *__restrict__ bound2,
                                                       unsigned char *__restrict__ mask, double *__restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (bound2) t2 = *bound2;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = F[k];
    const double e = epi_error(f, pts[i]);
    err[i] = e;
    mask[i] = (e <= t2 || (keep_all && *keep_all)) ? 1 : 0;
}

// ------------------------------------------------------------------ the LMedS filter
// An error is a non-negative double or +inf once a NaN counts as +inf, so errors order as their bit patterns do as unsigned
// integers: the key of an error.
constexpr u64 EPI_KEY_INF = 0x7ff0000000000000ull;
enum { I_PASSES = 20, I_PASSES1, I_MATCH_TILES, I_HIST_BYTES };               // info words of alp_epipolar_lmeds past the refit counts
enum { S_CHOSEN_VALUE = 0, S_FINAL_VALUE, S_BOUND2, S_REFIT_VALUE0 };         // stats words
static_assert(I_HIST_BYTES < EPI_INFO && S_REFIT_VALUE0 + EPI_MAX_REFITS <= EPI_LMEDS_STATS, "info or stats too short");

__device__ __forceinline__ u64 epi_key_of(double e) { return e != e ? EPI_KEY_INF : (u64)__double_as_longlong(e); }

// the key of e with one division, as epi_inlier forms e: s2 / min(a, b) = max(s2 / a, s2 / b) bit for bit.  Where the two
// differ, one is NaN and the other +inf (s2 = inf over one infinite divisor), which is one key.
__device__ __forceinline__ u64 epi_key(const double (&F)[9], const double4 q) {
    double ss, d2, d1;
    epi_terms(F, q.x, q.y, q.z, q.w, ss, d2, d1);
    double dm = d1 < d2 ? d1 : d2;
    if (d1 != d1) dm = d1;
    return epi_key_of(ss / dm);
}

// One pass: `shift` is the place of the pass' digit (60 in the first pass, 0 in the last).  prefix[h]: the digits above it
// (not read in the first pass); hist: the counters of this split, [16][h_pad] from its base.
__global__ __launch_bounds__(EPI_HYP_TILE) void epi_select_kernel(const double4 *__restrict__ pts, int n, const double *__restrict__ F, int H,
                                                                  int splits, long long match_tiles, long long h_pad,
                                                                  const u64 *__restrict__ prefix, int shift, unsigned *__restrict__ hist) {
    __shared__ double4 tile[EPI_MATCH_TILE];
    __shared__ unsigned cnt[EPI_SELECT_DIGITS * EPI_HYP_TILE];
    const long long htile = blockIdx.x / (unsigned)splits;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const long long h = htile * EPI_HYP_TILE + threadIdx.x;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = h < H ? F[(size_t)h * 9 + k] : nan64();
    const bool first = shift == 64 - EPI_SELECT_BITS;
    const u64 pre = first ? 0 : prefix[h];
    const u64 above = first ? 0 : ~(u64)0 << (shift + EPI_SELECT_BITS);
    unsigned *const mine = cnt + threadIdx.x;         // counter d at mine[d * 256]: no other lane touches it
#pragma unroll
    for (int d = 0; d < EPI_SELECT_DIGITS; ++d) mine[d * EPI_HYP_TILE] = 0;
    int64_t tb, te;
    match_split_range(match_tiles, splits, split, &tb, &te);
    for (long long t = tb; t < te; ++t) {
        const int base = (int)(t * EPI_MATCH_TILE);
        const int count = n - base < EPI_MATCH_TILE ? n - base : EPI_MATCH_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < count; i += EPI_HYP_TILE) tile[i] = pts[base + i];
        __syncthreads();
#pragma unroll 4
        for (int m = 0; m < count; ++m) {
            const u64 k = epi_key(f, tile[m]);
            if (((k ^ pre) & above) == 0) atomicAdd(mine + (int)((k >> shift) & (EPI_SELECT_DIGITS - 1)) * EPI_HYP_TILE, 1u);
        }
    }
    unsigned *const out = hist + (size_t)split * EPI_SELECT_DIGITS * h_pad + h;
#pragma unroll
    for (int d = 0; d < EPI_SELECT_DIGITS; ++d) out[(size_t)d * h_pad] = mine[d * EPI_HYP_TILE];
}

// a thread per padded hypothesis: the counters of the splits added in order, the digit at which they reach the remaining rank,
// the prefix extended by it and the rank reduced by what lies below it; after the last pass the prefix is the value
__global__ __launch_bounds__(256) void epi_select_merge_kernel(const unsigned *__restrict__ hist, int splits, long long h_pad, int H, int shift,
                                                               int rank0, u64 *__restrict__ prefix, int *__restrict__ rank,
                                                               double *__restrict__ value) {
    const long long h = (long long)blockIdx.x * 256 + threadIdx.x;
    if (h >= h_pad) return;
    const bool first = shift == 64 - EPI_SELECT_BITS;
    const unsigned r = (unsigned)(first ? rank0 : rank[h]);
    unsigned below = 0;
    int digit = EPI_SELECT_DIGITS - 1;
    for (int d = 0; d < EPI_SELECT_DIGITS; ++d) {
        unsigned c = 0;
        for (int s = 0; s < splits; ++s) c += hist[((size_t)s * EPI_SELECT_DIGITS + d) * h_pad + h];
        if (below + c >= r) {
            digit = d;
            break;
        }
        below += c;
    }
    const u64 p = (first ? 0 : prefix[h]) | (u64)digit << shift;
    prefix[h] = p;
    rank[h] = (int)(r - below);
    if (shift == 0 && h < H) value[h] = __longlong_as_double((long long)p);
}

// one workgroup: the smallest value, the lowest index on a tie (value and index do not pack into one 64-bit key: a
// lexicographic compare); the state of the filter from it
__global__ __launch_bounds__(256) void epi_lmeds_choose_kernel(const double *__restrict__ value, int H, const double *__restrict__ F, int rank,
                                                               double scale2, double floor2, EpiState *__restrict__ st) {
    __shared__ u64 bkey[256];
    __shared__ int bidx[256];
    u64 key = ~(u64)0;
    int idx = INT_MAX;
    for (int h = threadIdx.x; h < H; h += 256) {          // ascending h: a strict compare keeps the lowest index
        const u64 k = (u64)__double_as_longlong(value[h]);
        if (k < key) key = k, idx = h;
    }
    bkey[threadIdx.x] = key, bidx[threadIdx.x] = idx;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = 1; t < 256; ++t)
        if (bkey[t] < key || (bkey[t] == key && bidx[t] < idx)) key = bkey[t], idx = bidx[t];
    const double v = __longlong_as_double((long long)key);
    for (int k = 0; k < 9; ++k) st->Fcur[k] = F[(size_t)idx * 9 + k], st->Fcand[k] = nan64();
    for (int k = 0; k < EPI_INFO; ++k) st->info[k] = 0;
    for (int k = 0; k < EPI_MAX_REFITS; ++k) st->info[I_REFIT_COUNT0 + k] = -1;
    for (int k = 0; k < EPI_LMEDS_STATS; ++k) st->stats[k] = nan64();
    st->lmeds = 1, st->rank = rank, st->scale2 = scale2, st->floor2 = floor2;
    st->count = 0;
    st->keep_all = st->stopped = key < EPI_KEY_INF ? 0 : 1;
    const double sv = scale2 * v;
    st->value = v, st->bound2 = sv > floor2 ? sv : floor2;
    st->stats[S_CHOSEN_VALUE] = st->stats[S_FINAL_VALUE] = v, st->stats[S_BOUND2] = st->bound2;
    st->info[I_CHOSEN] = idx, st->info[I_KEEP_ALL] = st->keep_all;
}

// the keys of the errors of every match under the current F (candidate == 0) or the refit's candidate, with the mask
// kernel's arithmetic
__global__ __launch_bounds__(256) void epi_errs_kernel(const double4 *__restrict__ pts, int n, const EpiState *__restrict__ st, int candidate,
                                                       u64 *__restrict__ keys) {
    if (st->stopped) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = candidate ? st->Fcand[k] : st->Fcur[k];
    keys[i] = epi_key_of(epi_error(f, pts[i]));
}

// One workgroup over the keys of one F.  round < 0: the chosen hypothesis, whose value is known: the count of its inliers.
// Otherwise the candidate of refit `round`: its value by a radix select on the array (8-bit digits, integer LDS atomics: the
// counts do not depend on their order), its bound, its count, and the decision: it replaces the current F only when its value is
// strictly smaller, otherwise the loop stops.  A value that is not finite counts no inliers.
__global__ __launch_bounds__(EPI_SELECT1_BLOCK) void epi_lmeds_eval_kernel(const u64 *__restrict__ keys, int n, int round, EpiState *__restrict__ st) {
    __shared__ unsigned hist[256];
    __shared__ u64 s_prefix;
    __shared__ unsigned s_rank;
    __shared__ int red[EPI_SELECT1_BLOCK / 64];
    if (st->stopped) return;
    u64 vkey = (u64)__double_as_longlong(st->value);
    if (round >= 0) {
        u64 pre = 0;
        unsigned r = (unsigned)st->rank;
        for (int pass = 0; pass < EPI_SELECT1_PASSES; ++pass) {
            const int shift = 56 - 8 * pass;
            const u64 above = pass == 0 ? 0 : ~(u64)0 << (shift + 8);
            __syncthreads();
            if (threadIdx.x < 256) hist[threadIdx.x] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += EPI_SELECT1_BLOCK) {
                const u64 k = keys[i];
                if (((k ^ pre) & above) == 0) atomicAdd(hist + (int)((k >> shift) & 255), 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned below = 0;
                int digit = 255;
                for (int d = 0; d < 256; ++d) {
                    if (below + hist[d] >= r) {
                        digit = d;
                        break;
                    }
                    below += hist[d];
                }
                s_prefix = pre | (u64)digit << shift, s_rank = r - below;
            }
            __syncthreads();
            pre = s_prefix, r = s_rank;
        }
        vkey = pre;
    }
    const bool finite = vkey < EPI_KEY_INF;
    const double v = __longlong_as_double((long long)vkey);
    const double sv = st->scale2 * v, floor2 = st->floor2;
    const double b2 = sv > floor2 ? sv : floor2;
    const u64 bkey = (u64)__double_as_longlong(b2);           // b2 >= 0: e <= b2 is key <= its key (a NaN e has the key of +inf, and b2 is below it whenever v is finite and scale2 * v does not overflow)
    int c = 0;
    if (finite)
        for (int i = threadIdx.x; i < n; i += EPI_SELECT1_BLOCK) c += (keys[i] <= bkey && keys[i] < EPI_KEY_INF) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x != 0) return;
    c = 0;
    for (int w = 0; w < EPI_SELECT1_BLOCK / 64; ++w) c += red[w];
    if (round < 0) {
        st->count = c;
        st->info[I_CHOSEN_COUNT] = st->info[I_FINAL_COUNT] = c;
        return;
    }
    st->info[I_REFIT_COUNT0 + round] = c;
    st->info[I_REFITS_RUN] = round + 1;
    st->stats[S_REFIT_VALUE0 + round] = v;
    if (v < st->value) {
        for (int k = 0; k < 9; ++k) st->Fcur[k] = st->Fcand[k];
        st->count = c, st->value = v, st->bound2 = b2;
        st->info[I_FINAL_COUNT] = c;
        st->info[I_REFITS_KEPT] += 1;
        st->stats[S_FINAL_VALUE] = v, st->stats[S_BOUND2] = b2;
    } else {
        st->stopped = 1;
    }
}

// ------------------------------------------------------------------ alp_grid_thin
__global__ __launch_bounds__(256) void thin_dist_kernel(const long long *__restrict__ cell, const double *__restrict__ dist, long long n,
                                                        long long lo, u64 *__restrict__ best) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    atomicMin(best + (cell[i] - lo), (u64)__double_as_longlong(dist[i] + 0.0));       // (+ 0.0: a -0.0 orders as 0.0)
}
__global__ __launch_bounds__(256) void thin_index_kernel(const long long *__restrict__ cell, const double *__restrict__ dist, long long n,
                                                         long long lo, const u64 *__restrict__ best, u64 *__restrict__ first) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long c = cell[i] - lo;
    if (!dist || (u64)__double_as_longlong(dist[i] + 0.0) == best[c]) atomicMin(first + c, (u64)i);
}
__global__ __launch_bounds__(256) void thin_mask_kernel(const long long *__restrict__ cell, long long n, long long lo,
                                                        const u64 *__restrict__ first, unsigned char *__restrict__ mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mask[i] = first[cell[i] - lo] == (u64)i ? 1 : 0;
}

// ------------------------------------------------------------------ host side
struct EpiCall {
    host::EpiPlan p;
    DeviceBuffer<char> dev;
    char *d = nullptr;
    double4 *pts() const { return (double4 *)(d + p.off_pts); }
    int *samples() const { return (int *)(d + p.off_samples); }
    double *F() const { return (double *)(d + p.off_F); }
    int *partial() const { return (int *)(d + p.off_partial); }
    int *counts() const { return (int *)(d + p.off_counts); }
    EpiState *state() const { return (EpiState *)(d + p.off_state); }
    double *sym() const { return (double *)(d + p.off_sym); }
    int *cpart() const { return (int *)(d + p.off_cpart); }
    unsigned char *mask() const { return (unsigned char *)(d + p.off_mask); }
    double *err() const { return (double *)(d + p.off_err); }

    unsigned *hist() const { return (unsigned *)(d + p.off_hist); }
    u64 *prefix() const { return (u64 *)(d + p.off_prefix); }
    int *rank() const { return (int *)(d + p.off_rank); }
    double *value() const { return (double *)(d + p.off_value); }

    // with_select: the plan of the LMedS filter, which has the select's arrays after all the others
    int reserve(int64_t n, int64_t H, int splits, bool with_select = false) {
        p = with_select ? host::epi_select_plan(n, H, splits, ctx().cu_count) : host::epi_plan(n, H, splits, ctx().cu_count);
        if (int rc = dev.reserve(p.scratch_bytes)) return rc;
        d = dev;
        return ALP_OK;
    }
    // p1, p2 -> the packed matches and (with_norm) the normalisation in the state record
    hipError_t upload(const double *p1, const double *p2, int64_t n, bool with_norm) {
        hipStream_t st = ctx().stream;
        hipError_t e = hipMemcpyAsync(d + p.off_raw1, p1, (size_t)n * 16, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d + p.off_raw2, p2, (size_t)n * 16, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(state(), 0, EPI_STATE_BYTES, st);
        if (e != hipSuccess) return e;
        KTimeScope kt;
        hipLaunchKernelGGL(epi_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double2 *)(d + p.off_raw1),
                           (const double2 *)(d + p.off_raw2), (int)n, pts());
        if (with_norm) hipLaunchKernelGGL(epi_norm_kernel, dim3(1), dim3(256), 0, st, (const double4 *)pts(), (int)n, state());
        return hipGetLastError();
    }
    void launch_samples(int64_t n, int64_t H, uint64_t seed) {
        hipLaunchKernelGGL((epi_samples_kernel<EPI_SAMPLE, EPI_STREAM>), dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx().stream, (int)n, (int)H,
                           (unsigned)seed, (unsigned)(seed >> 32), samples());
    }
    // the essential filter: the call is planned for 10 H hypothesis slots, so the sample block holds the H rows of 5 and, from
    // byte 32 H on, the H solution counts
    int *nsol(int64_t H) const { return (int *)(d + p.off_samples + (size_t)H * 32); }
    void launch_samples5(int64_t n, int64_t H, uint64_t seed) {
        hipLaunchKernelGGL((epi_samples_kernel<EPI_SAMPLE5, EPI_STREAM5>), dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx().stream, (int)n,
                           (int)H, (unsigned)seed, (unsigned)(seed >> 32), samples());
    }
    void launch_solve5(int64_t H, const double K[3]) {
        hipLaunchKernelGGL(epi_essential_kernel, dim3(1), dim3(64), 0, ctx().stream, K[0], K[1], K[2], state());
        hipLaunchKernelGGL(epi_solve5_kernel, dim3((unsigned)((H + EPI_SOLVE_BLOCK - 1) / EPI_SOLVE_BLOCK)), dim3(EPI_SOLVE_BLOCK), 0, ctx().stream,
                           (const double4 *)pts(), (const int *)samples(), (int)H, (const EpiState *)state(), F(), nsol(H));
    }
    void launch_solve(int64_t H) {
        hipLaunchKernelGGL(epi_solve_kernel, dim3((unsigned)p.solve_blocks), dim3(EPI_SOLVE_BLOCK), 0, ctx().stream, (const double4 *)pts(),
                           (const int *)samples(), (int)H, (const EpiState *)state(), F());
    }
    void launch_score(int64_t n, int64_t H, double t2) {
        hipLaunchKernelGGL(epi_score_kernel, dim3((unsigned)p.workgroups), dim3(EPI_HYP_TILE), 0, ctx().stream, (const double4 *)pts(), (int)n,
                           (const double *)F(), (int)H, t2, p.splits, (long long)p.match_tiles, (long long)p.h_pad, partial());
        hipLaunchKernelGGL(epi_merge_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx().stream, (const int *)partial(), p.splits,
                           (long long)p.h_pad, (int)H, counts());
    }
    // value()[h] = the rank-th smallest error of hypothesis h: the passes of the select, each followed by its merge
    void launch_select(int64_t n, int64_t H, int rank) {
        for (int pass = 0; pass < p.passes; ++pass) {
            const int shift = 64 - EPI_SELECT_BITS * (pass + 1);
            hipLaunchKernelGGL(epi_select_kernel, dim3((unsigned)p.workgroups), dim3(EPI_HYP_TILE), 0, ctx().stream, (const double4 *)pts(), (int)n,
                               (const double *)F(), (int)H, p.splits, (long long)p.match_tiles, (long long)p.h_pad, (const u64 *)prefix(), shift, hist());
            hipLaunchKernelGGL(epi_select_merge_kernel, dim3((unsigned)(p.h_pad / 256)), dim3(256), 0, ctx().stream, (const unsigned *)hist(), p.splits,
                               (long long)p.h_pad, (int)H, shift, rank, prefix(), this->rank(), value());
        }
    }
};

// slots: hypotheses scored per sample (10 for the five-point solver, whose samples need 5 matches and not 8)
int epi_check_points(const char *fn, const double *p1, const double *p2, int64_t n, int64_t H, int slots = 1) {
    if (!p1 || !p2) return fail(ALP_EINVAL, "%s: NULL input", fn);
    const int64_t min_n = slots == 1 ? EPI_MIN_N : EPI_SAMPLE5, max_h = EPI_MAX_H / slots;
    if (n < min_n || n > EPI_MAX_N) return fail(ALP_EINVAL, "%s: n = %lld, must be %lld..2^20", fn, (long long)n, (long long)min_n);
    if (H < 1 || H > max_h) return fail(ALP_EINVAL, "%s: H = %lld, must be 1..%s", fn, (long long)H, slots == 1 ? "2^20" : "2^20 / 10");
    if (!host::epi_caps_ok(n, H * slots, min_n)) return fail(ALP_EINVAL, "%s: H * n = %lld * %lld passes 2^35 error evaluations", fn, (long long)H, (long long)n);
    return ALP_OK;
}

int epi_check_samples(const char *fn, const int32_t *samples, int64_t H, int64_t n, int width = EPI_SAMPLE) {
    for (int64_t i = 0; i < H * width; ++i)
        if (samples[i] < 0 || samples[i] >= n)
            return fail(ALP_EINVAL, "%s: sample %lld of hypothesis %lld is %d, outside 0..%lld", fn, (long long)(i % width),
                        (long long)(i / width), samples[i], (long long)(n - 1));
    return ALP_OK;
}

int epi_check_splits(const char *fn, int splits, int64_t n) {
    const int64_t tiles = (n + EPI_MATCH_TILE - 1) / EPI_MATCH_TILE;
    if (splits < 0) return fail(ALP_EINVAL, "%s: splits is negative", fn);
    if (splits > tiles)
        return fail(ALP_EINVAL, "%s: splits = %d, but %lld matches are only %lld tiles of %d", fn, splits, (long long)n, (long long)tiles,
                    EPI_MATCH_TILE);
    return ALP_OK;
}

int epi_check_K(const char *fn, const double *K) {
    if (!K) return fail(ALP_EINVAL, "%s: NULL K", fn);
    if (!(std::isfinite(K[0]) && K[0] > 0.0)) return fail(ALP_EINVAL, "%s: the focal length must be finite and positive", fn);
    if (!(std::isfinite(K[1]) && std::isfinite(K[2]))) return fail(ALP_EINVAL, "%s: the principal point must be finite", fn);
    return ALP_OK;
}

int epi_finish(const char *fn, hipError_t e) {
    const hipError_t es = hipStreamSynchronize(ctx().stream);          // before the device block and the caller's arrays go away
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ALP_EHIP, "%s: %s", fn, hipGetErrorString(e));
    return ALP_OK;
}

}  // namespace

extern "C" int alp_epipolar_samples(int64_t n, int64_t H, uint64_t seed, int32_t *samples) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(samples, "NULL output");
    ALP_REQUIRE(n >= EPI_MIN_N && n <= EPI_MAX_N, "n must be 8..2^20");
    ALP_REQUIRE(H >= 1 && H <= EPI_MAX_H, "H must be 1..2^20");
    DeviceBuffer<int> dev;
    if (int rc = dev.reserve((size_t)H * EPI_SAMPLE * 4)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e;
    {
        KTimeScope kt;
        hipLaunchKernelGGL((epi_samples_kernel<EPI_SAMPLE, EPI_STREAM>), dim3((unsigned)((H + 255) / 256)), dim3(256), 0, st, (int)n, (int)H,
                           (unsigned)seed, (unsigned)(seed >> 32), (int *)dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(samples, (int *)dev, (size_t)H * EPI_SAMPLE * 4, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_solve8(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, double *F) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H)) return rc;
    ALP_REQUIRE(samples && F, "NULL samples or output");
    if (int rc = epi_check_samples(__func__, samples, H, n)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H, 1)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, true);
    if (e == hipSuccess) e = hipMemcpyAsync(c.samples(), samples, (size_t)H * EPI_SAMPLE * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_solve(H);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(F, c.F(), (size_t)H * 72, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_score(const double *p1, const double *p2, int64_t n, const double *F, int64_t H, double threshold, int splits,
                                  int32_t *counts, int64_t info[6]) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H)) return rc;
    ALP_REQUIRE(F && counts, "NULL F or output");
    ALP_REQUIRE(std::isfinite(threshold) && threshold >= 0.0, "threshold must be finite and not negative");
    if (int rc = epi_check_splits(__func__, splits, n)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H, splits)) return rc;
    if (info) {
        info[0] = c.p.hyp_tile, info[1] = c.p.match_tile, info[2] = c.p.splits, info[3] = c.p.workgroups;
        info[4] = (int64_t)c.p.scratch_bytes, info[5] = c.p.match_tiles;
    }
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    if (e == hipSuccess) e = hipMemcpyAsync(c.F(), F, (size_t)H * 72, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_score(n, H, threshold * threshold);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(counts, c.counts(), (size_t)H * 4, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_mask(const double *p1, const double *p2, int64_t n, const double F[9], double threshold, uint8_t *mask,
                                 double *err) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, 1)) return rc;
    ALP_REQUIRE(F, "NULL F");
    ALP_REQUIRE(std::isfinite(threshold) && threshold >= 0.0, "threshold must be finite and not negative");
    EpiCall c;
    if (int rc = c.reserve(n, 1, 1)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    if (e == hipSuccess) e = hipMemcpyAsync(c.F(), F, 72, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        hipLaunchKernelGGL(epi_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double4 *)c.pts(), (int)n,
                           (const double *)c.F(), threshold * threshold, (const int *)nullptr, (const double *)nullptr, c.mask(), c.err());
        e = hipGetLastError();
    }
    if (e == hipSuccess && mask) e = hipMemcpyAsync(mask, c.mask(), (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && err) e = hipMemcpyAsync(err, c.err(), (size_t)n * 8, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

namespace {

// the whole filter: K == NULL the fundamental one on samples of 8, else the essential one on samples of 5 with 10 slots each
int epi_ransac(const char *fn, const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed, const double *K,
               double threshold, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24]) {
    if (int rc = require_init()) return rc;
    const int slots = K ? EPI_SLOTS5 : 1, width = K ? EPI_SAMPLE5 : EPI_SAMPLE;
    if (int rc = epi_check_points(fn, p1, p2, n, H, slots)) return rc;
    if (K)
        if (int rc = epi_check_K(fn, K)) return rc;
    if (!(std::isfinite(threshold) && threshold >= 0.0)) return fail(ALP_EINVAL, "%s: threshold must be finite and not negative", fn);
    if (!(refits >= 0 && refits <= EPI_MAX_REFITS)) return fail(ALP_EINVAL, "%s: refits must be 0..8", fn);
    if (int rc = epi_check_splits(fn, splits, n)) return rc;
    if (samples)
        if (int rc = epi_check_samples(fn, samples, H, n, width)) return rc;
    const int64_t HS = H * slots;       // hypothesis slots that are scored
    EpiCall c;
    if (int rc = c.reserve(n, HS, splits)) return rc;
    const double t2 = threshold * threshold;
    hipStream_t st = ctx().stream;
    EpiState host_state;
    hipError_t e = c.upload(p1, p2, n, !K);
    if (e == hipSuccess && samples) e = hipMemcpyAsync(c.samples(), samples, (size_t)H * width * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        // the whole filter is enqueued at once; what a round does is decided on the device (EpiState::stopped)
        KTimeScope kt;
        const double4 *pts = c.pts();
        EpiState *state = c.state();
        const unsigned rb = (unsigned)c.p.reduce_blocks;
        if (K) {
            if (!samples) c.launch_samples5(n, H, seed);
            c.launch_solve5(H, K);
        } else {
            if (!samples) c.launch_samples(n, H, seed);
            c.launch_solve(H);
        }
        c.launch_score(n, HS, t2);
        hipLaunchKernelGGL(epi_choose_kernel, dim3(1), dim3(256), 0, st, (const int *)c.counts(), (int)HS, (const double *)c.F(), width, state);
        for (int r = 0; r < refits; ++r) {
            hipLaunchKernelGGL(epi_accum_kernel, dim3(rb), dim3(EPI_REDUCE_BLOCK), 0, st, pts, (int)n, t2, (const EpiState *)state, c.sym());
            hipLaunchKernelGGL(epi_refit_kernel, dim3(1), dim3(64), 0, st, (const double *)c.sym(), (int)rb, state);
            hipLaunchKernelGGL(epi_count_kernel, dim3(rb), dim3(EPI_REDUCE_BLOCK), 0, st, pts, (int)n, t2, (const EpiState *)state, c.cpart());
            hipLaunchKernelGGL(epi_decide_kernel, dim3(1), dim3(64), 0, st, (const int *)c.cpart(), (int)rb, r, state);
        }
        hipLaunchKernelGGL(epi_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, (int)n, (const double *)state->Fcur, t2,
                           (const int *)&state->keep_all, (const double *)nullptr, c.mask(), c.err());
        e = hipGetLastError();
    }
    if (e == hipSuccess && mask) e = hipMemcpyAsync(mask, c.mask(), (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&host_state, c.state(), sizeof(EpiState), hipMemcpyDeviceToHost, st);
    if (int rc = epi_finish(fn, e)) return rc;
    if (F) memcpy(F, host_state.Fcur, 72);
    if (info) {
        for (int k = 0; k < EPI_INFO; ++k) info[k] = host_state.info[k];
        info[I_HYP_TILE] = c.p.hyp_tile, info[I_MATCH_TILE] = c.p.match_tile, info[I_SPLITS] = c.p.splits, info[I_WORKGROUPS] = c.p.workgroups;
        info[I_BYTES] = (int64_t)c.p.scratch_bytes, info[I_REDUCE_BLOCKS] = c.p.reduce_blocks;
    }
    return ALP_OK;
}

}  // namespace

extern "C" int alp_epipolar_ransac(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                                   double threshold, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24]) {
    return epi_ransac(__func__, p1, p2, n, samples, H, seed, nullptr, threshold, refits, splits, F, mask, info);
}

extern "C" int alp_essential_ransac(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                                    const double K[3], double threshold, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24]) {
    if (!K) return fail(ALP_EINVAL, "%s: NULL K", __func__);
    return epi_ransac(__func__, p1, p2, n, samples, H, seed, K, threshold, refits, splits, F, mask, info);
}

namespace {

// what the select adds to epi_check_points: the work of its passes, and the rank
int epi_check_select(const char *fn, int64_t n, int64_t H, int slots, int64_t rank) {
    if (!host::epi_select_caps_ok(n, H * slots, slots == 1 ? EPI_MIN_N : EPI_SAMPLE5))
        return fail(ALP_EINVAL, "%s: %d passes * H * n = %d * %lld * %lld pass 2^35 error evaluations", fn, EPI_SELECT_PASSES, EPI_SELECT_PASSES,
                    (long long)(H * slots), (long long)n);
    if (rank < 1 || rank > n) return fail(ALP_EINVAL, "%s: rank = %lld, must be 1..n = %lld", fn, (long long)rank, (long long)n);
    return ALP_OK;
}

// the LMedS filter: K == NULL the fundamental one, else the essential one
int epi_lmeds(const char *fn, const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed, const double *K,
              int64_t rank, double scale2, double floor2, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24], double stats[12]) {
    if (int rc = require_init()) return rc;
    const int slots = K ? EPI_SLOTS5 : 1, width = K ? EPI_SAMPLE5 : EPI_SAMPLE;
    if (int rc = epi_check_points(fn, p1, p2, n, H, slots)) return rc;
    if (int rc = epi_check_select(fn, n, H, slots, rank)) return rc;
    if (K)
        if (int rc = epi_check_K(fn, K)) return rc;
    if (!(std::isfinite(scale2) && scale2 >= 0.0)) return fail(ALP_EINVAL, "%s: scale2 must be finite and not negative", fn);
    if (!(std::isfinite(floor2) && floor2 >= 0.0)) return fail(ALP_EINVAL, "%s: floor2 must be finite and not negative", fn);
    if (!(refits >= 0 && refits <= EPI_MAX_REFITS)) return fail(ALP_EINVAL, "%s: refits must be 0..8", fn);
    if (int rc = epi_check_splits(fn, splits, n)) return rc;
    if (samples)
        if (int rc = epi_check_samples(fn, samples, H, n, width)) return rc;
    const int64_t HS = H * slots;
    EpiCall c;
    if (int rc = c.reserve(n, HS, splits, true)) return rc;
    hipStream_t st = ctx().stream;
    EpiState host_state;
    hipError_t e = c.upload(p1, p2, n, !K);
    if (e == hipSuccess && samples) e = hipMemcpyAsync(c.samples(), samples, (size_t)H * width * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        // enqueued at once, like epi_ransac: what a round does is decided on the device
        KTimeScope kt;
        const double4 *pts = c.pts();
        EpiState *state = c.state();
        u64 *keys = (u64 *)c.err();
        const unsigned rb = (unsigned)c.p.reduce_blocks, nb = (unsigned)((n + 255) / 256);
        if (K) {
            if (!samples) c.launch_samples5(n, H, seed);
            c.launch_solve5(H, K);
        } else {
            if (!samples) c.launch_samples(n, H, seed);
            c.launch_solve(H);
        }
        c.launch_select(n, HS, (int)rank);
        hipLaunchKernelGGL(epi_lmeds_choose_kernel, dim3(1), dim3(256), 0, st, (const double *)c.value(), (int)HS, (const double *)c.F(), (int)rank,
                           scale2, floor2, state);
        hipLaunchKernelGGL(epi_errs_kernel, dim3(nb), dim3(256), 0, st, pts, (int)n, (const EpiState *)state, 0, keys);
        hipLaunchKernelGGL(epi_lmeds_eval_kernel, dim3(1), dim3(EPI_SELECT1_BLOCK), 0, st, (const u64 *)keys, (int)n, -1, state);
        for (int r = 0; r < refits; ++r) {
            hipLaunchKernelGGL(epi_accum_kernel, dim3(rb), dim3(EPI_REDUCE_BLOCK), 0, st, pts, (int)n, 0.0, (const EpiState *)state, c.sym());
            hipLaunchKernelGGL(epi_refit_kernel, dim3(1), dim3(64), 0, st, (const double *)c.sym(), (int)rb, state);
            hipLaunchKernelGGL(epi_errs_kernel, dim3(nb), dim3(256), 0, st, pts, (int)n, (const EpiState *)state, 1, keys);
            hipLaunchKernelGGL(epi_lmeds_eval_kernel, dim3(1), dim3(EPI_SELECT1_BLOCK), 0, st, (const u64 *)keys, (int)n, r, state);
        }
        hipLaunchKernelGGL(epi_mask_kernel, dim3(nb), dim3(256), 0, st, pts, (int)n, (const double *)state->Fcur, 0.0, (const int *)&state->keep_all,
                           (const double *)&state->bound2, c.mask(), c.err());
        e = hipGetLastError();
    }
    if (e == hipSuccess && mask) e = hipMemcpyAsync(mask, c.mask(), (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&host_state, c.state(), sizeof(EpiState), hipMemcpyDeviceToHost, st);
    if (int rc = epi_finish(fn, e)) return rc;
    if (F) memcpy(F, host_state.Fcur, 72);
    if (info) {
        for (int k = 0; k < EPI_INFO; ++k) info[k] = host_state.info[k];
        info[I_HYP_TILE] = c.p.hyp_tile, info[I_MATCH_TILE] = c.p.match_tile, info[I_SPLITS] = c.p.splits, info[I_WORKGROUPS] = c.p.workgroups;
        info[I_BYTES] = (int64_t)c.p.scratch_bytes, info[I_REDUCE_BLOCKS] = c.p.reduce_blocks;
        info[I_PASSES] = c.p.passes, info[I_PASSES1] = EPI_SELECT1_PASSES, info[I_MATCH_TILES] = c.p.match_tiles;
        info[I_HIST_BYTES] = (int64_t)c.p.hist_bytes;
    }
    if (stats) memcpy(stats, host_state.stats, sizeof(host_state.stats));
    return ALP_OK;
}

}  // namespace

extern "C" int alp_epipolar_select(const double *p1, const double *p2, int64_t n, const double *F, int64_t H, int64_t rank, int splits,
                                   double *value, int64_t info[8]) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H)) return rc;
    if (int rc = epi_check_select(__func__, n, H, 1, rank)) return rc;
    ALP_REQUIRE(F && value, "NULL F or output");
    if (int rc = epi_check_splits(__func__, splits, n)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H, splits, true)) return rc;
    if (info) {
        info[0] = c.p.hyp_tile, info[1] = c.p.match_tile, info[2] = c.p.splits, info[3] = c.p.workgroups;
        info[4] = (int64_t)c.p.scratch_bytes, info[5] = c.p.match_tiles, info[6] = c.p.passes, info[7] = (int64_t)c.p.hist_bytes;
    }
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    if (e == hipSuccess) e = hipMemcpyAsync(c.F(), F, (size_t)H * 72, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_select(n, H, (int)rank);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(value, c.value(), (size_t)H * 8, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_lmeds(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed, int64_t rank,
                                  double scale2, double floor2, int refits, int splits, double F[9], uint8_t *mask, int64_t info[24],
                                  double stats[12]) {
    return epi_lmeds(__func__, p1, p2, n, samples, H, seed, nullptr, rank, scale2, floor2, refits, splits, F, mask, info, stats);
}

extern "C" int alp_essential_lmeds(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, uint64_t seed,
                                   const double K[3], int64_t rank, double scale2, double floor2, int refits, int splits, double F[9],
                                   uint8_t *mask, int64_t info[24], double stats[12]) {
    if (!K) return fail(ALP_EINVAL, "%s: NULL K", __func__);
    return epi_lmeds(__func__, p1, p2, n, samples, H, seed, K, rank, scale2, floor2, refits, splits, F, mask, info, stats);
}

extern "C" int alp_epipolar_samples5(int64_t n, int64_t H, uint64_t seed, int32_t *samples) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(samples, "NULL output");
    ALP_REQUIRE(n >= EPI_SAMPLE5 && n <= EPI_MAX_N, "n must be 5..2^20");
    ALP_REQUIRE(H >= 1 && H <= EPI_MAX_H, "H must be 1..2^20");
    DeviceBuffer<int> dev;
    if (int rc = dev.reserve((size_t)H * EPI_SAMPLE5 * 4)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e;
    {
        KTimeScope kt;
        hipLaunchKernelGGL((epi_samples_kernel<EPI_SAMPLE5, EPI_STREAM5>), dim3((unsigned)((H + 255) / 256)), dim3(256), 0, st, (int)n, (int)H,
                           (unsigned)seed, (unsigned)(seed >> 32), (int *)dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(samples, (int *)dev, (size_t)H * EPI_SAMPLE5 * 4, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_epipolar_solve5(const double *p1, const double *p2, int64_t n, const int32_t *samples, int64_t H, const double K[3],
                                   double *F, int32_t *nsol) {
    if (int rc = require_init()) return rc;
    if (int rc = epi_check_points(__func__, p1, p2, n, H, EPI_SLOTS5)) return rc;
    ALP_REQUIRE(samples && F && nsol, "NULL samples or output");
    if (int rc = epi_check_K(__func__, K)) return rc;
    if (int rc = epi_check_samples(__func__, samples, H, n, EPI_SAMPLE5)) return rc;
    EpiCall c;
    if (int rc = c.reserve(n, H * EPI_SLOTS5, 1)) return rc;
    hipStream_t st = ctx().stream;
    hipError_t e = c.upload(p1, p2, n, false);
    if (e == hipSuccess) e = hipMemcpyAsync(c.samples(), samples, (size_t)H * EPI_SAMPLE5 * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        c.launch_solve5(H, K);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(F, c.F(), (size_t)H * EPI_SLOTS5 * 72, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nsol, c.nsol(H), (size_t)H * 4, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}

extern "C" int alp_grid_thin(const int64_t *cell_id, const double *dist, int64_t n, uint8_t *mask) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(n >= 0 && n <= THIN_MAX_N, "n must be 0..2^30");
    if (n == 0) return ALP_OK;
    ALP_REQUIRE(cell_id && mask, "NULL input or output");
    int64_t lo = cell_id[0], hi = cell_id[0];
    for (int64_t i = 1; i < n; ++i) lo = std::min(lo, cell_id[i]), hi = std::max(hi, cell_id[i]);
    // (unsigned: the difference of two int64 may pass INT64_MAX)
    if ((uint64_t)hi - (uint64_t)lo >= (uint64_t)THIN_MAX_SPAN)
        return fail(ALP_EINVAL, "alp_grid_thin: cell ids span %lld..%lld, more than 2^26 cells", (long long)lo, (long long)hi);
    if (dist)
        for (int64_t i = 0; i < n; ++i)
            if (!(dist[i] >= 0.0)) return fail(ALP_EINVAL, "alp_grid_thin: dist[%lld] is negative or NaN", (long long)i);
    const size_t span = (size_t)(hi - lo) + 1;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    const size_t off_cell = take((size_t)n * 8), off_dist = take(dist ? (size_t)n * 8 : 0), off_tables = take(span * 16), off_mask = take((size_t)n);
    DeviceBuffer<char> dev;
    if (int rc = dev.reserve(at)) return rc;
    char *d = dev;
    long long *cell_dev = (long long *)(d + off_cell);
    double *dist_dev = dist ? (double *)(d + off_dist) : nullptr;
    u64 *best = (u64 *)(d + off_tables), *first = best + span;
    hipStream_t st = ctx().stream;
    hipError_t e = hipMemcpyAsync(cell_dev, cell_id, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && dist) e = hipMemcpyAsync(dist_dev, dist, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(best, 0xff, span * 16, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        const dim3 grid((unsigned)((n + 255) / 256));
        if (dist) hipLaunchKernelGGL(thin_dist_kernel, grid, dim3(256), 0, st, (const long long *)cell_dev, (const double *)dist_dev, (long long)n, (long long)lo, best);
        hipLaunchKernelGGL(thin_index_kernel, grid, dim3(256), 0, st, (const long long *)cell_dev, (const double *)dist_dev, (long long)n, (long long)lo,
                           (const u64 *)best, first);
        hipLaunchKernelGGL(thin_mask_kernel, grid, dim3(256), 0, st, (const long long *)cell_dev, (long long)n, (long long)lo, (const u64 *)first,
                           (unsigned char *)(d + off_mask));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(mask, d + off_mask, (size_t)n, hipMemcpyDeviceToHost, st);
    return epi_finish(__func__, e);
}
