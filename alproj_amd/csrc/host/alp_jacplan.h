// The derivative of the fold (fold_pose_jacobian) and the plan jacobian_kernel / normal_poses_kernel read (jacobian_plan), written
// once for the host and the device: a forward-mode dual number run through fold_pose_any of host/alp_fold.h.
// host/alp_host.cpp wraps them as the host functions of host/alp_host.h (argument checks and error texts stay there, the
// results bit for bit); the device loop of the least-squares iteration (alp_lm.hip) builds the plan of every trial point on
// the GPU with the same code, one lane per target.  Included by host/alp_host.h after JacPlan; nothing here may include a HIP
// header (ALP_HD is empty outside a HIP compilation).
#pragma once

namespace alp {

// A forward-mode dual number: v + d eps with eps^2 = 0.  fold_pose_any<Dual> carries d rec / d theta_j next to rec when
// theta_j is seeded with d = 1.
struct Dual {
    double v, d;
    ALP_HD Dual(double v_ = 0, double d_ = 0) : v(v_), d(d_) {}
    ALP_HD Dual &operator+=(const Dual &b) { v += b.v; d += b.d; return *this; }
};
ALP_HD inline Dual operator-(const Dual &a) { return Dual(-a.v, -a.d); }
ALP_HD inline Dual operator+(const Dual &a, const Dual &b) { return Dual(a.v + b.v, a.d + b.d); }
ALP_HD inline Dual operator+(const Dual &a, double b) { return Dual(a.v + b, a.d); }
ALP_HD inline Dual operator+(double a, const Dual &b) { return Dual(a + b.v, b.d); }
ALP_HD inline Dual operator-(const Dual &a, const Dual &b) { return Dual(a.v - b.v, a.d - b.d); }
ALP_HD inline Dual operator-(const Dual &a, double b) { return Dual(a.v - b, a.d); }
ALP_HD inline Dual operator-(double a, const Dual &b) { return Dual(a - b.v, -b.d); }
ALP_HD inline Dual operator*(const Dual &a, const Dual &b) { return Dual(a.v * b.v, a.d * b.v + a.v * b.d); }
ALP_HD inline Dual operator*(const Dual &a, double b) { return Dual(a.v * b, a.d * b); }
ALP_HD inline Dual operator*(double a, const Dual &b) { return Dual(a * b.v, a * b.d); }
ALP_HD inline Dual operator/(const Dual &a, const Dual &b) { return Dual(a.v / b.v, (a.d * b.v - a.v * b.d) / (b.v * b.v)); }
ALP_HD inline Dual operator/(const Dual &a, double b) { return Dual(a.v / b, a.d / b); }
ALP_HD inline Dual operator/(double a, const Dual &b) { return Dual(a / b.v, -a * b.d / (b.v * b.v)); }
ALP_HD inline Dual fold_sin(const Dual &a) { return Dual(std::sin(a.v), std::cos(a.v) * a.d); }
ALP_HD inline Dual fold_cos(const Dual &a) { return Dual(std::cos(a.v), -std::sin(a.v) * a.d); }
ALP_HD inline Dual fold_tan(const Dual &a) {
    const double t = std::tan(a.v);
    return Dual(t, (1 + t * t) * a.d);
}

// the lens word of each lens parameter (a1 .. s4 = indices 7 .. 20), as fold_pose_any writes them; -1: no lens parameter
ALP_HD inline int jac_lens_word(int param) {
    return param == 7 ? 18 : param == 8 ? 19 : (param >= 9 && param <= 14) ? param + 3 : (param >= 15 && param <= 20) ? param + 5 : -1;
}

// d rec[0 .. POSE_WORDS) / d params[target], the derivative of the very arithmetic fold_pose does
ALP_HD inline void fold_pose_derivative_hd(const double params[ALP_NPARAM], const double origin[3], int target, Dual rec[POSE_WORDS]) {
    Dual p[ALP_NPARAM];
    for (int i = 0; i < ALP_NPARAM; ++i) p[i] = Dual(params[i], i == target ? 1.0 : 0.0);
    fold_pose_any<Dual>(p, params[21], params[22], origin, rec);
}

// fold_pose_jacobian without its checks: jac[m * D + j] = d rec[m] / d params[target[j]], m < JAC_WORDS
ALP_HD inline void fold_pose_jacobian_hd(const double params[ALP_NPARAM], const double origin[3], const int32_t *target, int D, double *jac) {
    Dual rec[POSE_WORDS];
    for (int j = 0; j < D; ++j) {
        fold_pose_derivative_hd(params, origin, target[j], rec);
        for (int m = 0; m < JAC_WORDS; ++m) jac[m * D + j] = rec[m].d;
    }
}

// jacobian_plan in two parts, so that the targets can be shared out: the head (everything but the entries of the targets; the
// entries are zeroed) ...
ALP_HD inline void jacobian_plan_head_hd(const double params[ALP_NPARAM], const double origin[3], int D, int of_residuals, JacPlan *plan) {
    fold_pose_hd(params, origin, plan->rec);
    for (int j = 0; j < JAC_MAX; ++j) {
        for (int k = 0; k < 12; ++k) plan->drow[j][k] = 0.0;
        plan->lens_f[j] = 0.0;
        plan->lens_w[j] = 0;
    }
    plan->D = D;
    plan->su = of_residuals ? -plan->rec[26] : plan->rec[26];
    plan->sv = of_residuals ? -plan->rec[27] : plan->rec[27];
}

// ... and the entry of target j (drow[j] or lens_f[j], and lens_w[j])
ALP_HD inline void jacobian_plan_target_hd(const double params[ALP_NPARAM], const double origin[3], int target, int j, JacPlan *plan) {
    Dual rec[POSE_WORDS];
    fold_pose_derivative_hd(params, origin, target, rec);
    const int m = jac_lens_word(target);
    plan->lens_w[j] = m < 0 ? -1 : m - 12;
    if (m < 0)
        for (int k = 0; k < 12; ++k) plan->drow[j][k] = rec[k].d;
    else
        plan->lens_f[j] = rec[m].d;
}

// jacobian_plan without its checks
ALP_HD inline void jacobian_plan_hd(const double params[ALP_NPARAM], const double origin[3], const int32_t *target, int D, int of_residuals,
                                    JacPlan *plan) {
    jacobian_plan_head_hd(params, origin, D, of_residuals, plan);
    for (int j = 0; j < D; ++j) jacobian_plan_target_hd(params, origin, target[j], j, plan);
}

}  // namespace alp
