// icp_gicp_math.h -- the per-correspondence fp64 routines of the plane-to-plane (generalized) ICP (icp.hip, umereg_icp_gicp.h): the weight
// W = (C_q + R C_s R^T)^-1 of a correspondence from the two normals, and its terms of the 6x6 normal equations.  Not part of the C ABI.
//
// GICP's regularised covariance of a locally planar point (eigenvalues (eps, 1, 1) in the frame of its normal n) is a function of the
// normal alone, C = I - (1 - eps) n n^T, so with a = R n_s and b = n_q
//     M = C_q + R C_s R^T = 2 I - (1 - eps) (a a^T + b b^T),
// symmetric positive definite with eigenvalues in [2 eps, 2] for unit (or zero) normals: cond(M) <= 1 / eps.
#pragma once
// UMEREG_ICP_GICP_HOST: the same text as plain C++, for a test harness that judges the routines on the CPU (tests/icp_gicp_host.cpp);
// the device build does not define it.
#ifdef UMEREG_ICP_GICP_HOST
#define UMEREG_GICP_FN inline
#else
#include "common.h"
#define UMEREG_GICP_FN __device__ inline
#endif

namespace umereg {

// W = M^-1 (upper triangle {xx, xy, xz, yy, yz, zz}) by cofactors: M is 3x3 and its condition number is bounded by 1 / eps, so the
// closed form errs by a few cond(M) 2^-53 relative to max |W|.  Even in a and in b: only a a^T and b b^T enter.  A zero normal is an
// isotropic covariance for that point; eps = 1 gives M = 2 I whatever the normals are.
UMEREG_GICP_FN void gicp_weight(const double (&a)[3], const double (&b)[3], double eps, double (&W)[6])
{
    const double k = 1.0 - eps;
    const double m00 = 2.0 - k * (a[0] * a[0] + b[0] * b[0]);
    const double m01 = 0.0 - k * (a[0] * a[1] + b[0] * b[1]);
    const double m02 = 0.0 - k * (a[0] * a[2] + b[0] * b[2]);
    const double m11 = 2.0 - k * (a[1] * a[1] + b[1] * b[1]);
    const double m12 = 0.0 - k * (a[1] * a[2] + b[1] * b[2]);
    const double m22 = 2.0 - k * (a[2] * a[2] + b[2] * b[2]);
    const double c00 = m11 * m22 - m12 * m12;
    const double c01 = m02 * m12 - m01 * m22;
    const double c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02;
    const double c12 = m01 * m02 - m00 * m12;
    const double c22 = m00 * m11 - m01 * m01;
    const double inv = 1.0 / (m00 * c00 + m01 * c01 + m02 * c02);
    W[0] = c00 * inv; W[1] = c01 * inv; W[2] = c02 * inv;
    W[3] = c11 * inv; W[4] = c12 * inv; W[5] = c22 * inv;
}

// s[0..20] += the upper triangle (row by row) of J0^T W J0, s[21..26] += J0^T W d, for one correspondence: p the transformed source
// point, d = p - q, J0 = [ -[p]x  I3 ] (3x6) the derivative of the moved point in open3d's six parameters (rotation first), so that
// J0^T = [ G ; I3 ] with G = [p]x, G v = p x v.  In blocks: J0^T W J0 = [ G W G^T, G W ; (G W)^T, W ] and J0^T W d = [ G W d ; W d ].
// With W = n n^T these are the point-to-plane terms J J^T and J r, J = [p x n, n].
UMEREG_GICP_FN void gicp_accumulate(const double (&p)[3], const double (&d)[3], const double (&W)[6], double* s)
{
    const double Wf[3][3] = {{W[0], W[1], W[2]}, {W[1], W[3], W[4]}, {W[2], W[4], W[5]}};
    double GW[3][3];   // G W: column c is p x (column c of W)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        GW[0][c] = p[1] * Wf[2][c] - p[2] * Wf[1][c];
        GW[1][c] = p[2] * Wf[0][c] - p[0] * Wf[2][c];
        GW[2][c] = p[0] * Wf[1][c] - p[1] * Wf[0][c];
    }
    // (G W G^T)[r][c] = (row r of G W) . (row c of G) = (p x row r of G W)[c]; rows of the upper triangle start at 0, 6, 11, 15, 18, 20
    s[0] += GW[0][2] * p[1] - GW[0][1] * p[2];
    s[1] += GW[0][0] * p[2] - GW[0][2] * p[0];
    s[2] += GW[0][1] * p[0] - GW[0][0] * p[1];
    s[6] += GW[1][0] * p[2] - GW[1][2] * p[0];
    s[7] += GW[1][1] * p[0] - GW[1][0] * p[1];
    s[11] += GW[2][1] * p[0] - GW[2][0] * p[1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s[3 + c] += GW[0][c];
        s[8 + c] += GW[1][c];
        s[12 + c] += GW[2][c];
    }
    s[15] += W[0]; s[16] += W[1]; s[17] += W[2];
    s[18] += W[3]; s[19] += W[4];
    s[20] += W[5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        s[21 + r] += GW[r][0] * d[0] + GW[r][1] * d[1] + GW[r][2] * d[2];
        s[24 + r] += Wf[r][0] * d[0] + Wf[r][1] * d[1] + Wf[r][2] * d[2];
    }
}

}  // namespace umereg
