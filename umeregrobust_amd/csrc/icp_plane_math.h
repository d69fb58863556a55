// icp_plane_math.h -- the small dense fp64 routines of the point-to-plane ICP (icp.hip) and of the normal estimation (normals.hip):
// a cyclic Jacobi eigen-solver for symmetric 3x3 / 6x6 matrices, the normal of a 3x3 covariance, the thresholded solve of the 6x6
// normal equations and open3d's TransformVector6dToMatrix4d.  Not part of the C ABI.
#pragma once
// UMEREG_ICP_PLANE_HOST: the same text as plain C++, for a test harness that judges the routines on the CPU (tests/icp_plane_host.cpp);
// the device build does not define it.
#ifdef UMEREG_ICP_PLANE_HOST
#include <cmath>
#define UMEREG_PLANE_FN inline
#else
#include "common.h"
#define UMEREG_PLANE_FN __device__ inline
#endif

namespace umereg {

constexpr double kSymJacobiTol = 4.0e-16;   // a_pq^2 <= tol^2 |a_pp a_qq|: the pair is diagonal to working precision
constexpr int kSymJacobiSweeps = 24;
constexpr double kPlaneRankTol = 1.0e-12;   // eigenvalues <= this * lambda_max of J^T J count as zero (minimum-norm solution)

// Cyclic two-sided Jacobi for a symmetric N x N matrix: on return A holds the eigenvalues on its diagonal and the columns of V are the
// (orthonormal) eigenvectors.  The stop test is relative to the two diagonal entries (the matrices here are sums of outer products:
// |a_pq|^2 <= a_pp a_qq), so an eigenvector errs by ~ u |A| / gap.  A pair whose off-diagonal entry is exactly zero is never rotated:
// rows and columns that are exactly zero stay exactly zero, and V keeps the unit vectors of those axes.
template <int N>
UMEREG_PLANE_FN void sym_jacobi(double (&A)[N][N], double (&V)[N][N])
{
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
        for (int q = 0; q < N; ++q) V[p][q] = p == q ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSymJacobiSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < N - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                if (apq * apq <= (kSymJacobiTol * kSymJacobiTol) * fabs(app * aqq)) continue;
                rotated = true;
                const double zeta = (aqq - app) / (2.0 * apq);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                A[p][p] = app - t * apq;
                A[q][q] = aqq + t * apq;
                A[p][q] = 0.0;
                A[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < N; ++r) {
                    if (r != p && r != q) {
                        const double arp = A[r][p], arq = A[r][q];
                        const double np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
                        A[r][p] = np_; A[p][r] = np_;
                        A[r][q] = nq_; A[q][r] = nq_;
                    }
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
            }
        if (!rotated) break;
    }
}

// The normal of a neighbourhood from the upper triangle of its 3x3 covariance (any positive scale) {xx, xy, xz, yy, yz, zz}: the unit
// eigenvector of the smallest eigenvalue, sign made canonical (the component of largest magnitude is positive; ties -> the lowest
// axis).  A zero covariance gives (0, 0, 1), open3d's rule for a neighbourhood without a plane.
UMEREG_PLANE_FN void covariance_normal(const double (&c)[6], double (&n)[3])
{
    if (c[0] == 0.0 && c[1] == 0.0 && c[2] == 0.0 && c[3] == 0.0 && c[4] == 0.0 && c[5] == 0.0) {
        n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
        return;
    }
    double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}}, V[3][3];
    sym_jacobi<3>(A, V);
    double v[3] = {V[0][0], V[1][0], V[2][0]};
    double lam = A[0][0];
    if (A[1][1] < lam) { lam = A[1][1]; v[0] = V[0][1]; v[1] = V[1][1]; v[2] = V[2][1]; }
    if (A[2][2] < lam) { lam = A[2][2]; v[0] = V[0][2]; v[1] = V[1][2]; v[2] = V[2][2]; }
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(len > 0.0)) {   // (not reached with an orthonormal V; NaN input lands here)
        n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
        return;
    }
    int big = 0;
    if (fabs(v[1]) > fabs(v[big])) big = 1;
    if (fabs(v[2]) > fabs(v[big])) big = 2;
    const double sgn = (big == 0 ? v[0] : big == 1 ? v[1] : v[2]) < 0.0 ? -1.0 : 1.0;
    n[0] = sgn * v[0] / len; n[1] = sgn * v[1] / len; n[2] = sgn * v[2] / len;
}

// x = -pinv(A) b for the symmetric positive semi-definite A = sum J J^T (upper triangle, row by row: 21 entries) and b = sum J r:
// eigenvalues at or below kPlaneRankTol * lambda_max are treated as zero, so a rank-deficient system (a single wall, a ground plane)
// gets the minimum-norm solution -- the directions the correspondences do not constrain are left untouched.  (open3d solves with
// Eigen's LDLT; the two agree wherever A has full rank.)  A zero or non-finite A gives x = 0.
UMEREG_PLANE_FN void plane_solve(const double (&au)[21], const double (&b)[6], double (&x)[6])
{
    double A[6][6], V[6][6];
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q) {
            A[p][q] = au[k];
            A[q][p] = au[k];
            ++k;
        }
    sym_jacobi<6>(A, V);
    double lmax = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) lmax = A[p][p] > lmax ? A[p][p] : lmax;
#pragma unroll
    for (int r = 0; r < 6; ++r) x[r] = 0.0;
    if (!(lmax > 0.0)) return;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const double lam = A[p][p];
        if (!(lam > kPlaneRankTol * lmax)) continue;
        double vb = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) vb += V[r][p] * b[r];
        const double w = vb / lam;
#pragma unroll
        for (int r = 0; r < 6; ++r) x[r] -= V[r][p] * w;
    }
}

// open3d's TransformVector6dToMatrix4d: R = Rz(x[2]) Ry(x[1]) Rx(x[0]), t = x[3..5]
UMEREG_PLANE_FN void euler_update(const double (&x)[6], double (&R)[3][3], double (&t)[3])
{
    const double sx = sin(x[0]), cx = cos(x[0]), sy = sin(x[1]), cy = cos(x[1]), sz = sin(x[2]), cz = cos(x[2]);
    R[0][0] = cz * cy; R[0][1] = cz * sy * sx - sz * cx; R[0][2] = cz * sy * cx + sz * sx;
    R[1][0] = sz * cy; R[1][1] = sz * sy * sx + cz * cx; R[1][2] = sz * sy * cx - cz * sx;
    R[2][0] = -sy;     R[2][1] = cy * sx;                R[2][2] = cy * cx;
    t[0] = x[3]; t[1] = x[4]; t[2] = x[5];
}

}  // namespace umereg
