// Part of alp_epipolar.hip (one translation unit, included inside its anonymous namespace after epi_dev.h; not a stand-alone
// header): hypothesis generation -- the minimal samples, the normalised 8-point solve, the five-point solver, and the
// rank-2 / essential projection and denormalisation that the refit shares with them.
//
//   epi_samples_kernel    a thread per hypothesis: 8 (the essential filter: 5, on a stream word of their own) distinct indices
//                         from the counter-based generator of alp_sampler.h keyed by (seed, hypothesis, attempt); a repeat is
//                         rejected and the next draw taken
//   epi_solve_kernel      a thread per hypothesis, 64 per workgroup.  The 8 x 9 matrix of the normalised sample lives in LDS, element
//                         e of lane l at e * 64 + l (72 doubles indexed by a pivot search would otherwise go to scratch); Gaussian
//                         elimination with complete pivoting, the null vector by back substitution, rank 2 by a one-sided Jacobi
//                         sweep over the three columns, T2^T F T1, unit Frobenius norm.  Rank below 8 or a non-finite F: NaN.
//   epi_solve5_kernel     the essential filter (reference gcp.py:200-252): a thread per sample of 5 matches, 64 per workgroup, Nister's
//                         five-point solver -> up to 10 essential matrices per sample as pixel-space matrices K^-T E K^-1, which
//                         everything below scores, chooses and refits like any other hypothesis (10 slots per sample, NaN = unused);
//                         the refit then projects onto the essential matrices (EpiState::essential).  Details at the kernel.
#pragma once

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
