// quat_f64.h — fp64 rotations for the kernels that compute in double and round once: quaternions (w, x, y, z) for the
// evaluation's forward kinematics (eval_metrics.h) and the motion windows (motion_windows.h), Rodrigues' matrix for the body
// model (body_model.h) and the AMASS joints (amass_prep.h).  (The prefix kernel's Quat helpers in pointwise.h are fp32.)
#pragma once
#include "common.h"

struct QuatD {
    double w, x, y, z;
};
EG_D QuatD qd_mul(QuatD a, QuatD b) {
    return QuatD{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                 a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
EG_D QuatD qd_std(QuatD q) { return q.w < 0.0 ? QuatD{-q.w, -q.x, -q.y, -q.z} : q; }
// (cos(a / 2), sin(a / 2) / a * v), the factors from their series below 1e-6
EG_D QuatD qd_from_aa(double x, double y, double z) {
    const double a2 = x * x + y * y + z * z;
    double s, c;
    if (a2 < 1e-12) {
        s = 0.5 - a2 / 48.0;
        c = 1.0 - a2 / 8.0;
    } else {
        const double a = sqrt(a2);
        s = sin(0.5 * a) / a;
        c = cos(0.5 * a);
    }
    return qd_std(QuatD{c, x * s, y * s, z * s});
}
// p + w t + q.xyz x t with t = 2 q.xyz x p (unit q)
EG_D void qd_rotate(QuatD q, const double (&p)[3], double (&o)[3]) {
    const double tx = 2.0 * (q.y * p[2] - q.z * p[1]), ty = 2.0 * (q.z * p[0] - q.x * p[2]), tz = 2.0 * (q.x * p[1] - q.y * p[0]);
    o[0] = p[0] + q.w * tx + (q.y * tz - q.z * ty);
    o[1] = p[1] + q.w * ty + (q.z * tx - q.x * tz);
    o[2] = p[2] + q.w * tz + (q.x * ty - q.y * tx);
}

// R = I + (sin a / a) K + ((1 - cos a) / a^2) K^2, a = |v|; the two factors from their series below 1e-6 (exact at v = 0)
EG_D void rodrigues(double x, double y, double z, double (&R)[9]) {
    const double a2 = x * x + y * y + z * z;
    double s, c;
    if (a2 < 1e-12) {
        s = 1.0 - a2 / 6.0;
        c = 0.5 - a2 / 24.0;
    } else {
        const double a = sqrt(a2), h = sin(0.5 * a);
        s = sin(a) / a;
        c = 2.0 * h * h / a2;
    }
    R[0] = 1.0 - c * (y * y + z * z); R[1] = c * x * y - s * z;         R[2] = c * x * z + s * y;
    R[3] = c * x * y + s * z;         R[4] = 1.0 - c * (x * x + z * z); R[5] = c * y * z - s * x;
    R[6] = c * x * z - s * y;         R[7] = c * y * z + s * x;         R[8] = 1.0 - c * (x * x + y * y);
}
