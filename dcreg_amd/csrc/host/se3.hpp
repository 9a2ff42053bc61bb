// SE(3) state helpers of the engine: MathUtils::exp / SE3State::boxplus (DCReg/include/math_utils.hpp:20-33,
// 158-166), Pose6D2Matrix / calculatePoseError (DCReg/include/utils.hpp:452-460, 497-535).
#pragma once
#include <cmath>
#include <cstring>

namespace dcreg {

inline void mat3mul(const double *A, const double *B, double *C) {
    double o[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
        o[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
    std::memcpy(C, o, sizeof(o));
}

// so(3) -> SO(3), Rodrigues; first-order for |w| < 1e-10 exactly like the reference
inline void so3Exp(const double w[3], double R[9]) {
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (th < 1e-10) {
        const double S[9] = {1, -w[2], w[1], w[2], 1, -w[0], -w[1], w[0], 1};
        std::memcpy(R, S, sizeof(S));
        return;
    }
    const double ax = w[0] / th, ay = w[1] / th, az = w[2] / th;
    const double K[9] = {0, -az, ay, az, 0, -ax, -ay, ax, 0};
    double KK[9];
    mat3mul(K, K, KK);
    const double s = std::sin(th), c1 = 1.0 - std::cos(th);
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + s * K[i] + c1 * KK[i];
}

// se(3) -> SE(3) (include/dcreg.h, deskew): xi = (w, v), theta = |w|, R = I + A W + B W^2, t = (I + B W + C W^2) v with W = [w]x; below
// theta = 1e-3 the coefficients are their series through theta^4.  deskew.hip evaluates the same expression on the device.
inline void se3Coeffs(double th2, double th, double &A, double &B, double &Cc) {
    if (th < 1e-3) {
        A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
        B = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
        Cc = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
    } else {
        const double s = std::sin(th), c = std::cos(th);
        A = s / th;
        B = (1.0 - c) / th2;
        Cc = (th - s) / (th2 * th);
    }
}
inline void se3Exp(const double xi[6], double R[9], double t[3]) {
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th2 = wx * wx + wy * wy + wz * wz, th = std::sqrt(th2);
    double A, B, Cc;
    se3Coeffs(th2, th, A, B, Cc);
    const double W[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double W2[9], V[9];
    mat3mul(W, W, W2);
    for (int i = 0; i < 9; ++i) {
        const double I = i % 4 == 0 ? 1.0 : 0.0;
        R[i] = I + A * W[i] + B * W2[i];
        V[i] = I + B * W[i] + Cc * W2[i];
    }
    for (int i = 0; i < 3; ++i) t[i] = V[i * 3] * xi[3] + V[i * 3 + 1] * xi[4] + V[i * 3 + 2] * xi[5];
}

// SE(3) -> se(3), the inverse of se3Exp for rotations below pi: w = angle-axis of R (theta = atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2)),
// v = V^-1 t with V^-1 = I - W / 2 + D W^2, D = (1 - A / (2 B)) / theta^2 (series below theta = 1e-3).  Returns theta.
inline double se3Log(const double R[9], const double t[3], double xi[6]) {
    const double s[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double sn = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const double th = std::atan2(sn, 0.5 * (R[0] + R[4] + R[8] - 1.0));
    const double th2 = th * th;
    const double f = th < 1e-3 ? 1.0 + th2 / 6.0 + 7.0 * th2 * th2 / 360.0 : th / sn;
    for (int a = 0; a < 3; ++a) xi[a] = f * s[a];
    double D;
    if (th < 1e-3) {
        D = 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0;
    } else {
        double A, B, Cc;
        se3Coeffs(th2, th, A, B, Cc);
        D = (1.0 - A / (2.0 * B)) / th2;
    }
    const double W[9] = {0, -xi[2], xi[1], xi[2], 0, -xi[0], -xi[1], xi[0], 0};
    double W2[9];
    mat3mul(W, W, W2);
    for (int i = 0; i < 3; ++i) {
        double v = 0.0;
        for (int j = 0; j < 3; ++j) v += ((i == j ? 1.0 : 0.0) - 0.5 * W[i * 3 + j] + D * W2[i * 3 + j]) * t[j];
        xi[3 + i] = v;
    }
    return th;
}

// right perturbation: R <- R exp(w), t <- t + R v
inline void boxplus(const double R[9], const double t[3], const double dx[6], double Ro[9], double to[3]) {
    double E[9], Rn[9], tn[3];
    so3Exp(dx, E);
    mat3mul(R, E, Rn);
    for (int i = 0; i < 3; ++i) tn[i] = t[i] + R[i * 3] * dx[3] + R[i * 3 + 1] * dx[4] + R[i * 3 + 2] * dx[5];
    std::memcpy(Ro, Rn, sizeof(Rn));
    std::memcpy(to, tn, sizeof(tn));
}

// Translation * Rz(yaw) * Ry(pitch) * Rx(roll), row-major 4x4
inline void pose6dToMatrix(double roll, double pitch, double yaw, double x, double y, double z, double T[16]) {
    const double cr = std::cos(roll), sr = std::sin(roll), cp = std::cos(pitch), sp = std::sin(pitch);
    const double cy = std::cos(yaw), sy = std::sin(yaw);
    const double Rx[9] = {1, 0, 0, 0, cr, -sr, 0, sr, cr};
    const double Ry[9] = {cp, 0, sp, 0, 1, 0, -sp, 0, cp};
    const double Rz[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1};
    double A[9], B[9];
    mat3mul(Rz, Ry, A);
    mat3mul(A, Rx, B);
    for (int i = 0; i < 16; ++i) T[i] = 0.0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i * 4 + j] = B[i * 3 + j];
    T[3] = x; T[7] = y; T[11] = z; T[15] = 1.0;
}

inline void stateToMatrix(const double R[9], const double t[3], double T[16]) {
    for (int i = 0; i < 16; ++i) T[i] = 0.0;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) T[i * 4 + j] = R[i * 3 + j]; T[i * 4 + 3] = t[i]; }
    T[15] = 1.0;
}

// E = gt^-1 * T ; translation norm ; rotation angle as Eigen::AngleAxisd(R_E).angle() (through a quaternion)
inline void poseError(const double gt[16], const double T[16], double *trans, double *rotDeg) {
    double E[9], te[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += gt[k * 4 + i] * T[k * 4 + j];
            E[i * 3 + j] = s;
        }
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += gt[k * 4 + i] * (T[k * 4 + 3] - gt[k * 4 + 3]);
        te[i] = s;
    }
    *trans = std::sqrt(te[0] * te[0] + te[1] * te[1] + te[2] * te[2]);
    double q[4];   // w x y z
    const double tr = E[0] + E[4] + E[8];
    if (tr > 0.0) {
        double s = std::sqrt(tr + 1.0);
        q[0] = 0.5 * s; s = 0.5 / s;
        q[1] = (E[7] - E[5]) * s; q[2] = (E[2] - E[6]) * s; q[3] = (E[3] - E[1]) * s;
    } else {
        int i = 0;
        if (E[4] > E[0]) i = 1;
        if (E[8] > E[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = std::sqrt(E[i * 4] - E[j * 4] - E[k * 4] + 1.0);
        q[1 + i] = 0.5 * s; s = 0.5 / s;
        q[0] = (E[k * 3 + j] - E[j * 3 + k]) * s;
        q[1 + j] = (E[j * 3 + i] + E[i * 3 + j]) * s;
        q[1 + k] = (E[k * 3 + i] + E[i * 3 + k]) * s;
    }
    const double n = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double ang = n != 0.0 ? 2.0 * std::atan2(n, std::fabs(q[0])) : 0.0;
    *rotDeg = std::fabs(ang) * 180.0 / M_PI;
}

}  // namespace dcreg
