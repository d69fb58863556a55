// polar_grad.h -- the derivative of polar.h's rotation with respect to its 3x3 input, for rtume_grad.hip.  Not part of the C ABI.
// Compiles as plain C++ under UMEREG_POLAR_HOST, like polar.h.
#pragma once
#include "polar.h"

namespace umereg {

// The singular frames polar_rotation(A, R) builds its R from, by the same Hestenes sweeps in the same order:
//     R = u0 v0^T + u1 v1^T + u2 v2^T,   u2 = u0 x u1,  v2 = v0 x v1,   U[i][:] = u_i,  V[i][:] = v_i,
// and the signed values s[i] = u_i^T A v_i of the unscaled A: s[0] >= s[1] >= |s[2]|, s[2] = det(U_svd Vh_svd) * sigma_3, because
// both frames are right-handed as built.  -> false where polar_rotation returns R = I without looking at A (A zero, infinite or
// NaN); U, V, s are not written then.
UMEREG_POLAR_FN bool polar_frames(const double A[3][3], double U[3][3], double V[3][3], double s[3])
{
    double amax = 0.0;
    bool nan = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            amax = fmax(amax, fabs(A[p][q]));
            nan |= A[p][q] != A[p][q];
        }
    if (!(amax > 0.0) || !(amax <= 1.7976931348623157e308) || nan) return false;
    const int sh = -ilogb(amax);
    double As[3][3], W[3][3], Vj[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) W[p][q] = As[p][q] = ldexp(A[p][q], sh);
    for (int sweep = 0; sweep < kPolarSweeps; ++sweep) {
        bool any = hestenes_rotate<0, 1>(W, Vj);
        any |= hestenes_rotate<0, 2>(W, Vj);
        any |= hestenes_rotate<1, 2>(W, Vj);
        if (!any) break;
    }
    const double l0 = W[0][0] * W[0][0] + W[1][0] * W[1][0] + W[2][0] * W[2][0];
    const double l1 = W[0][1] * W[0][1] + W[1][1] * W[1][1] + W[2][1] * W[2][1];
    const double l2 = W[0][2] * W[0][2] + W[1][2] * W[1][2] + W[2][2] * W[2][2];
    const int i_min = (l0 <= l1 && l0 <= l2) ? 0 : ((l1 <= l2) ? 1 : 2);
    double* v0 = V[0];
    double* v1 = V[1];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        v0[r] = i_min == 0 ? Vj[r][1] : Vj[r][0];
        v1[r] = i_min == 2 ? Vj[r][1] : Vj[r][2];
    }
    const double la = i_min == 0 ? l1 : l0, lb = i_min == 2 ? l1 : l2;
    if (lb > la) {
#pragma unroll
        for (int r = 0; r < 3; ++r) { const double tmp = v0[r]; v0[r] = v1[r]; v1[r] = tmp; }
    }
    double* u0 = U[0];
    double* u1 = U[1];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u0[r] = As[r][0] * v0[0] + As[r][1] * v0[1] + As[r][2] * v0[2];
        u1[r] = As[r][0] * v1[0] + As[r][1] * v1[1] + As[r][2] * v1[2];
    }
    const double n0 = sqrt(u0[0] * u0[0] + u0[1] * u0[1] + u0[2] * u0[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u0[r] /= n0;
    const double d01 = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
    const double n1_raw = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] -= d01 * u0[r];
    double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    // rank 1, as polar.h declares it: u1 is completed arbitrarily, and R is no function of A in that direction
    if (!(n1 > 1e-150) || !(n1 > 1e-8 * n1_raw)) {
        const int ax = (fabs(u0[0]) <= fabs(u0[1]) && fabs(u0[0]) <= fabs(u0[2])) ? 0
                       : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
        double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
        cross3(u0, e, u1);
        n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] /= n1;
    const double d01b = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] -= d01b * u0[r];
    const double n1b = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] /= n1b;
    cross3(u0, u1, U[2]);
    cross3(v0, v1, V[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p) t += U[i][p] * (A[p][0] * V[i][0] + A[p][1] * V[i][1] + A[p][2] * V[i][2]);
        s[i] = t;
    }
    return true;
}

// gA = d <gR, R(A)> / dA for R = polar_rotation(A), the derivative of the rotation itself, from the frames and signed values of
// polar_frames(A, U, V, s):
//     C = U^T gR V,   Y_ij = (C_ij - C_ji) / (s_i + s_j)  (i != j),   gA = U Y V^T = sum_{i<j} Y_ij (u_i v_j^T - u_j v_i^T).
// No 1 / (s_i^2 - s_j^2): repeated singular values are no singularity of R; only s_i + s_j -> 0 is (i, j = 1, 2: the second and
// the signed third value cancel, a reflection as good as a rotation).  A pair with s_i + s_j <= min_gap * s_0 gets Y_ij = 0 (so
// does a NaN sum).
UMEREG_POLAR_FN void polar_rotation_grad(const double U[3][3], const double V[3][3], const double s[3], const double gR[3][3],
                                         double min_gap, double gA[3][3])
{
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) gA[p][q] = 0.0;
    double C[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 3; ++p) t += U[i][p] * (gR[p][0] * V[j][0] + gR[p][1] * V[j][1] + gR[p][2] * V[j][2]);
            C[i][j] = t;
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = i + 1; j < 3; ++j) {
            const double gap = s[i] + s[j];
            const double y = gap > min_gap * s[0] ? (C[i][j] - C[j][i]) / gap : 0.0;
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) gA[p][q] += y * (U[i][p] * V[j][q] - U[j][p] * V[i][q]);
        }
}

}  // namespace umereg
