// The bounded Levenberg-Marquardt iteration on the normal equations (alproj_amd/optimize.py: _normal_lm_steps, the iteration
// behind LsqOptimizer.optimize(method="normal"), reference driver src/alproj/optimize.py:442-539) as a state machine on plain
// data, written once for the host and the device.  _normal_lm_steps is the specification, statement by statement; normal_lm's
// docstring is its prose.  One LmState per start; three functions:
//   lm_start    the generator's opening lines: x0 clipped into the box is the first trial point, with no step
//   lm_consume  "consume the sums at the trial point": the first evaluation (scale, mu_0; status -1 when anything is not
//               finite), or accept / reject, gain ratio, Nielsen update and the f / x stopping tests
//   lm_produce  "produce the next trial point or stop": gtol and max_nfev tests, the free set, the damped matrix scaled to a
//               unit diagonal, Cholesky, two triangular solves, clip into the box, the predicted reduction of the clipped step;
//               a failed factorisation or a non-positive prediction raises the damping and tries again until mu is not finite
// A caller alternates them: lm_start, then { evaluate at s->trial; lm_consume; if still running lm_produce } until
// s->phase == LM_STOPPED.  The linear algebra is serial here, so that the host can run the whole machine
// (host/alp_host_selfcheck.cpp --lm, tests/test_lm_device_host.py); the device loop (alp_lm.hip) runs this very code.
// Same operations in the same order as the Python, one rounding each: every translation unit that includes this for its
// arithmetic is compiled with -ffp-contract=off.  Included by host/alp_host.h; nothing here may include a HIP header.
#pragma once

namespace alp {

constexpr int LM_MAX_D = JAC_MAX;                               // 23 targets: alp_normal_equations' limit
constexpr int LM_TRI = LM_MAX_D * (LM_MAX_D + 1) / 2;           // 276: the packed upper triangle of G
constexpr int LM_WORK = LM_MAX_D * LM_MAX_D + 4 * LM_MAX_D;     // doubles of scratch lm_produce needs
constexpr int LM_RUNNING = -2;                                  // LmState::status of a start that has not stopped (no stop uses it)

enum { LM_FIRST = 0, LM_TRIAL = 1, LM_STOPPED = 2 };            // LmState::phase: what the pending evaluation is, or none

struct LmConfig {
    double lower[LM_MAX_D], upper[LM_MAX_D];                    // either may be infinite
    double ftol, xtol, gtol;
    int32_t D, max_nfev;
};

struct alignas(8) LmState {
    double x[LM_MAX_D];           // the current point
    double G[LM_TRI];             // J^T J there: row-major upper triangle, alp_normal_equations' layout
    double g[LM_MAX_D];           // J^T r there
    double scale[LM_MAX_D];       // running maximum of sqrt(diag G)
    double trial[LM_MAX_D];       // the pending trial point
    double step[LM_MAX_D];        // trial - x, clipped
    double cost, mu, nu, predicted;
    int32_t nfev, iterations, status, phase;
};

ALP_HD inline int lm_tri_index(int D, int i, int j) {            // i <= j
    return i * D - i * (i - 1) / 2 + (j - i);
}
ALP_HD inline double lm_G(const double *G, int D, int i, int j) { return i <= j ? G[lm_tri_index(D, i, j)] : G[lm_tri_index(D, j, i)]; }
ALP_HD inline bool lm_finite(double v) { return v - v == 0.0; }
ALP_HD inline double lm_clip(double v, double lo, double hi) {   // np.clip: minimum(maximum(v, lo), hi); NaN stays NaN
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}
ALP_HD inline double lm_norm(const double *v, int D) {
    double s = 0.0;
    for (int i = 0; i < D; ++i) s += v[i] * v[i];
    return std::sqrt(s);
}
// ~(((x <= lower) & (g > 0)) | ((x >= upper) & (g < 0)))
ALP_HD inline bool lm_free(const LmConfig &c, const LmState *s, int i) {
    return !((s->x[i] <= c.lower[i] && s->g[i] > 0) || (s->x[i] >= c.upper[i] && s->g[i] < 0));
}
// the infinity norm of g over the free variables (0 when none is free); NaN for a start that failed at x0
ALP_HD inline double lm_grad_norm(const LmConfig &c, const LmState *s) {
    if (s->status == -1) return NAN;
    double m = 0.0;
    for (int i = 0; i < c.D; ++i)
        if (lm_free(c, s, i)) {
            const double a = std::fabs(s->g[i]);
            m = a > m ? a : m;
        }
    return m;
}

ALP_HD inline void lm_stop(LmState *s, int status) {
    s->status = status;
    s->phase = LM_STOPPED;
}

ALP_HD inline void lm_start(const LmConfig &c, const double *x0, LmState *s) {
    for (int i = 0; i < LM_MAX_D; ++i) s->x[i] = s->g[i] = s->scale[i] = s->trial[i] = s->step[i] = 0.0;
    for (int i = 0; i < LM_TRI; ++i) s->G[i] = 0.0;
    for (int i = 0; i < c.D; ++i) s->x[i] = s->trial[i] = lm_clip(x0[i], c.lower[i], c.upper[i]);
    s->cost = 0.0;
    s->mu = 0.0;
    s->nu = 2.0;
    s->predicted = -1.0;
    s->nfev = s->iterations = 0;
    s->status = LM_RUNNING;
    s->phase = LM_FIRST;
}

// G (packed), g, cost: the sums at s->trial
ALP_HD inline void lm_consume(const LmConfig &c, LmState *s, const double *G, const double *g, double cost) {
    const int D = c.D, tri = D * (D + 1) / 2;
    bool finite = lm_finite(cost);
    for (int i = 0; i < tri; ++i) finite = finite && lm_finite(G[i]);
    for (int i = 0; i < D; ++i) finite = finite && lm_finite(g[i]);
    if (s->phase == LM_FIRST) {
        s->nfev = 1;
        s->iterations = 0;
        if (!finite) {
            s->cost = cost;
            lm_stop(s, -1);
            return;
        }
        for (int i = 0; i < tri; ++i) s->G[i] = G[i];
        for (int i = 0; i < D; ++i) s->g[i] = g[i];
        s->cost = cost;
        double top = lm_G(G, D, 0, 0);
        for (int i = 0; i < D; ++i) {
            const double d = lm_G(G, D, i, i);
            s->scale[i] = std::sqrt(d);
            top = d > top ? d : top;
        }
        s->mu = 1e-3 * top;
        s->nu = 2.0;
        if (!(s->mu > 0)) s->mu = 1e-3;
        s->phase = LM_TRIAL;          // running: lm_produce follows
        return;
    }
    s->nfev += 1;
    const double actual = s->cost - cost;
    const double step_norm = lm_norm(s->step, D), x_norm = lm_norm(s->x, D);
    const bool accepted = finite && cost < s->cost;
    const double ratio = accepted ? actual / s->predicted : -1.0;
    const bool f_stop = accepted && actual < c.ftol * s->cost && ratio > 0.25;
    const bool x_stop = step_norm < c.xtol * (c.xtol + x_norm);
    if (accepted) {
        for (int i = 0; i < D; ++i) s->x[i] = s->trial[i];
        for (int i = 0; i < tri; ++i) s->G[i] = G[i];
        for (int i = 0; i < D; ++i) s->g[i] = g[i];
        s->cost = cost;
        s->iterations += 1;
        const double f = 1.0 - std::pow(2.0 * ratio - 1.0, 3.0);
        s->mu = s->mu * (1.0 / 3.0 > f ? 1.0 / 3.0 : f);
        s->nu = 2.0;
    } else {
        s->mu = s->mu * s->nu;
        s->nu = s->nu * 2.0;
    }
    if (f_stop || x_stop) lm_stop(s, (f_stop && x_stop) ? 4 : (f_stop ? 2 : 3));
}

// the next trial point into s->trial (s->phase stays LM_TRIAL), or a stop.  `work`: LM_WORK doubles of scratch.
ALP_HD inline void lm_produce(const LmConfig &c, LmState *s, double *work) {
    const int D = c.D;
    double *A = work, *jv = work + LM_MAX_D * LM_MAX_D, *rhs = jv + LM_MAX_D, *Gs = rhs + LM_MAX_D;
    int idx[LM_MAX_D];
    while (true) {
        int nf = 0;
        double g_norm = 0.0;
        for (int i = 0; i < D; ++i)
            if (lm_free(c, s, i)) {
                idx[nf++] = i;
                const double a = std::fabs(s->g[i]);
                g_norm = a > g_norm ? a : g_norm;
            }
        if (g_norm < c.gtol) return lm_stop(s, 1);
        if (s->nfev >= c.max_nfev) return lm_stop(s, 0);
        double top = 0.0;
        for (int i = 0; i < D; ++i) {
            const double q = std::sqrt(lm_G(s->G, D, i, i));
            s->scale[i] = (q > s->scale[i] || q != q) ? q : s->scale[i];      // np.maximum: NaN wins
            const double s2 = s->scale[i] * s->scale[i];
            top = (i == 0 || s2 > top) ? s2 : top;
        }
        // A = G[free, free] + diag(mu * (scale[free]^2 / top)), then scaled to a unit diagonal: A * outer(j, j)
        bool ok = true;
        for (int a = 0; a < nf; ++a) {
            const double s2 = s->scale[idx[a]] * s->scale[idx[a]];
            const double dA = lm_G(s->G, D, idx[a], idx[a]) + s->mu * (top > 0 ? s2 / top : 1.0);
            A[a * LM_MAX_D + a] = dA;
            ok = ok && dA > 0;
        }
        if (ok) {
            for (int a = 0; a < nf; ++a) jv[a] = 1.0 / std::sqrt(A[a * LM_MAX_D + a]);
            for (int a = 0; a < nf; ++a)
                for (int b = 0; b <= a; ++b) {
                    const double v = a == b ? A[a * LM_MAX_D + a] : lm_G(s->G, D, idx[a], idx[b]);
                    A[a * LM_MAX_D + b] = v * (jv[a] * jv[b]);
                }
            // Cholesky (lower, in place, row by row); a pivot that is not positive is a failed step
            for (int a = 0; a < nf && ok; ++a) {
                for (int b = 0; b <= a; ++b) {
                    double v = A[a * LM_MAX_D + b];
                    for (int k = 0; k < b; ++k) v -= A[a * LM_MAX_D + k] * A[b * LM_MAX_D + k];
                    if (b < a) {
                        A[a * LM_MAX_D + b] = v / A[b * LM_MAX_D + b];
                    } else {
                        if (!(v > 0) || !lm_finite(v)) ok = false;
                        A[a * LM_MAX_D + a] = std::sqrt(v);
                    }
                }
            }
        }
        if (ok) {
            // delta = -j * solve(L^T, solve(L, j * g[free]))
            for (int a = 0; a < nf; ++a) {
                double v = jv[a] * s->g[idx[a]];
                for (int k = 0; k < a; ++k) v -= A[a * LM_MAX_D + k] * rhs[k];
                rhs[a] = v / A[a * LM_MAX_D + a];
            }
            for (int a = nf - 1; a >= 0; --a) {
                double v = rhs[a];
                for (int k = a + 1; k < nf; ++k) v -= A[k * LM_MAX_D + a] * rhs[k];
                rhs[a] = v / A[a * LM_MAX_D + a];
            }
            for (int a = 0; a < nf; ++a) {
                rhs[a] = -jv[a] * rhs[a];
                ok = ok && lm_finite(rhs[a]);
            }
        }
        double predicted = -1.0;
        if (ok) {
            for (int i = 0; i < D; ++i) s->step[i] = 0.0;
            for (int a = 0; a < nf; ++a) s->step[idx[a]] = rhs[a];
            for (int i = 0; i < D; ++i) {
                s->trial[i] = lm_clip(s->x[i] + s->step[i], c.lower[i], c.upper[i]);
                s->step[i] = s->trial[i] - s->x[i];
            }
            // predicted = -(g @ step + 0.5 * (step @ G @ step)), the reduction of the clipped step
            double gs = 0.0, sGs = 0.0;
            for (int i = 0; i < D; ++i) gs += s->g[i] * s->step[i];
            for (int j = 0; j < D; ++j) {
                double v = 0.0;
                for (int i = 0; i < D; ++i) v += s->step[i] * lm_G(s->G, D, i, j);
                Gs[j] = v;
            }
            for (int j = 0; j < D; ++j) sGs += Gs[j] * s->step[j];
            predicted = -(gs + 0.5 * sGs);
        }
        if (!ok || !(predicted > 0)) {
            // no usable step at this damping.  Once mu dwarfs G, the step is -g / mu scaled: when even that is below xtol, stop
            if (ok && lm_norm(s->step, D) < c.xtol * (c.xtol + lm_norm(s->x, D))) return lm_stop(s, 3);
            s->mu = s->mu * s->nu;
            s->nu = s->nu * 2.0;
            if (!lm_finite(s->mu)) return lm_stop(s, 3);
            continue;
        }
        s->predicted = predicted;
        s->phase = LM_TRIAL;
        return;
    }
}

// one whole transition on the sums at the pending point: consume, then produce while the start goes on
ALP_HD inline void lm_advance(const LmConfig &c, LmState *s, const double *G, const double *g, double cost, double *work) {
    lm_consume(c, s, G, g, cost);
    if (s->phase != LM_STOPPED) lm_produce(c, s, work);
}

}  // namespace alp
