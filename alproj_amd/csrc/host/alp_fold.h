// The float64 folding of a camera pose (fold_pose) and its lens-free form (lens_free_from_general), written once for the host
// and the device; the fold is a template on its scalar type so that its derivative (fold_pose_jacobian) is the same code.  host/alp_host.cpp wraps them as the host functions of host/alp_host.h, compiled as before; the device loop
// of the CMA-ES generation (alp_cma.hip) folds every candidate of a generation on the GPU with the same code.  Included by
// host/alp_host.h after POSE_WORDS; nothing here may include a HIP header (ALP_HD is empty outside a HIP compilation).
#pragma once

#include <cmath>

#include "alproj_hip.h"

#if defined(__HIP__)
#define ALP_HD __host__ __device__
#else
#define ALP_HD
#endif

namespace alp {

// Reference arithmetic being folded (all float64, src/alproj/optimize.py):
//   intrinsic_mat :35-38   fov_x = fov*pi/180; fov_y = fov_x*h/w (Q5);
//                          fx = w/(2 tan(fov_x/2)); fy = h/(2 tan(fov_y/2))
//   extrinsic_mat :71-95   R = Rx(-(tilt+90)) . Ry(-roll) . Rz(pan);  t = R.(-cam)
//   project :144-149       cam = R.p + t;  (x,y,z) = K.cam;  u = w - x/z (Q4);  v = y/z
//   _distort :104-106      c = float32((w-1)/2, (h-1)/2);  x1 = (u-c0)/c0;  y1 = (v-c1)/c1
// With p = origin + q:  cam = R.q + R.(origin - cam_pos), and
//   x1 = ((w-c0)/c0) - (x/z)/c0 = ( ((w-c0)/c0).rowZ - rowx/c0 ) . [q;1] / (rowZ.[q;1])
//   y1 = (y/z)/c1 - 1          = ( rowy/c1 - rowZ ) . [q;1] / (rowZ.[q;1])
// where rowx = fx.R0 + cx.R2, rowy = fy.R1 + cy.R2, rowZ = R2 (4-vectors incl. translation).
// The principal-point cancellation (cx.Z against c0.Z) therefore happens here in float64.
// The trigonometric functions of the fold, overloaded on its scalar type (host/alp_host.cpp adds them for its dual number)
ALP_HD inline double fold_sin(double a) { return std::sin(a); }
ALP_HD inline double fold_cos(double a) { return std::cos(a); }
ALP_HD inline double fold_tan(double a) { return std::tan(a); }

// The fold on any scalar type T that has the arithmetic of double: T = double is fold_pose_hd below (every record the kernels
// read), T = a forward-mode dual number is its derivative (host/alp_host.cpp: fold_pose_jacobian).  w and h stay double: they
// are no targets, and they reach c0 / c1 through a float32 rounding.
template <typename T>
ALP_HD inline void fold_pose_any(const T p[ALP_NPARAM], double w, double h, const double origin[3], T rec[POSE_WORDS]) {
    const T X = p[0], Y = p[1], Z = p[2], fov = p[3], pan_d = p[4], tilt_d = p[5],
            roll_d = p[6];
    const T cx = p[23], cy = p[24];
    const double pi = M_PI;

    const T fov_x = fov * pi / 180;
    const T fov_y = fov_x * h / w;
    const T fx = w / (2 * fold_tan(fov_x / 2));
    const T fy = h / (2 * fold_tan(fov_y / 2));

    const T a = pan_d * pi / 180;
    const T b = -(tilt_d + 90) * pi / 180;
    const T c = -roll_d * pi / 180;
    const T rz[3][3] = {{fold_cos(a), -fold_sin(a), 0}, {fold_sin(a), fold_cos(a), 0}, {0, 0, 1}};
    const T rx[3][3] = {{1, 0, 0}, {0, fold_cos(b), -fold_sin(b)}, {0, fold_sin(b), fold_cos(b)}};
    const T ry[3][3] = {{fold_cos(c), 0, fold_sin(c)}, {0, 1, 0}, {-fold_sin(c), 0, fold_cos(c)}};
    T rxy[3][3], R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            T s = 0;
            for (int k = 0; k < 3; ++k) s += rx[i][k] * ry[k][j];
            rxy[i][j] = s;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            T s = 0;
            for (int k = 0; k < 3; ++k) s += rxy[i][k] * rz[k][j];
            R[i][j] = s;
        }
    const T d[3] = {origin[0] - X, origin[1] - Y, origin[2] - Z};
    T row[3][4];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) row[i][j] = R[i][j];
        row[i][3] = R[i][0] * d[0] + R[i][1] * d[1] + R[i][2] * d[2];
    }
    const double c0 = (double)(float)((w - 1) / 2);
    const double c1 = (double)(float)((h - 1) / 2);
    const double A = (w - c0) / c0;
    for (int j = 0; j < 4; ++j) {
        const T rowx = fx * row[0][j] + cx * row[2][j];
        const T rowy = fy * row[1][j] + cy * row[2][j];
        rec[0 + j] = A * row[2][j] - rowx / c0;
        rec[4 + j] = rowy / c1 - row[2][j];
        rec[8 + j] = row[2][j];
    }
    for (int i = 0; i < 6; ++i) rec[12 + i] = p[9 + i];   // k1..k6
    rec[18] = 1 + p[7];                                    // 1 + a1
    rec[19] = 1 + p[8];                                    // 1 + a2
    rec[20] = 2 * p[15];                                   // 2 p1
    rec[21] = 2 * p[16];                                   // 2 p2
    for (int i = 0; i < 4; ++i) rec[22 + i] = p[17 + i];  // s1..s4
    rec[26] = c0;
    rec[27] = c1;
    rec[28] = -c0;                                         // residual = (uo - c0) + (-c0) * x1_d
    rec[29] = -c1;
    rec[30] = rec[31] = 0;
}

ALP_HD inline void fold_pose_hd(const double p[ALP_NPARAM], const double origin[3], double rec[POSE_WORDS]) {
    fold_pose_any<double>(p, p[21], p[22], origin, rec);
}

ALP_HD inline void lens_free_from_general_hd(const double g[POSE_WORDS], double rec[POSE_WORDS]) {
    const double sy = g[18] / g[19];               // (1 + a1) / (1 + a2)  (a2 = -1: inf / NaN rows, and losses, like the reference's division)
    for (int i = 0; i < POSE_WORDS; ++i) rec[i] = 0;
    for (int j = 0; j < 4; ++j) {
        rec[0 + j] = g[28] * g[0 + j];             // -c0 X'
        rec[4 + j] = (g[29] * sy) * g[4 + j];      // -c1 (1 + a1) / (1 + a2) Y'
        rec[8 + j] = g[8 + j];
    }
    rec[26] = g[26];
    rec[27] = g[27];
}

}  // namespace alp
