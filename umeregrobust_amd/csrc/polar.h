// polar.h -- 3x3 polar rotation (one-sided Jacobi SVD of A), shared by rtume.hip and icp.hip.  Not part of the C ABI.
#pragma once
// UMEREG_POLAR_HOST: the same text as plain C++, for a test harness that judges the routine on the CPU; the device build does not define it.
#ifdef UMEREG_POLAR_HOST
#include <cmath>
#define UMEREG_POLAR_FN inline
#define UMEREG_POLAR_FN_INLINE inline
#else
#include "common.h"
#define UMEREG_POLAR_FN __device__ inline
#define UMEREG_POLAR_FN_INLINE __device__ __forceinline__
#endif

namespace umereg {

constexpr double kPolarTol = 4.0e-16;   // |w_p . w_q| <= tol |w_p| |w_q|: the columns are orthogonal
constexpr int kPolarSweeps = 12;

// One step of the one-sided (Hestenes) Jacobi SVD: rotate columns P, Q of W = A V (and of V) so that they become orthogonal.
// Works on A itself, never on A^T A: the rotations are orthogonal updates of A's columns, so the computed pairs are exact for
// an A + dA with |dA| ~ u |A| and the rotation errs by ~ u |A| / (s2 + det s3), the problem's own sensitivity.  (An eigen-solve
// of A^T A squares the spectrum: u (s1/s2)^2, 1e-5 for a cross-moment as thin as one lidar ring.)
// -> true if the pair needed a rotation.
template <int P, int Q>
UMEREG_POLAR_FN_INLINE bool hestenes_rotate(double (&W)[3][3], double (&V)[3][3])
{
    const double alpha = W[0][P] * W[0][P] + W[1][P] * W[1][P] + W[2][P] * W[2][P];
    const double beta = W[0][Q] * W[0][Q] + W[1][Q] * W[1][Q] + W[2][Q] * W[2][Q];
    const double gamma = W[0][P] * W[0][Q] + W[1][P] * W[1][Q] + W[2][P] * W[2][Q];
    // orthogonal to working precision (also: a zero column, an exactly diagonal input)
    if (gamma * gamma <= (kPolarTol * kPolarTol) * (alpha * beta)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double wp = W[r][P], wq = W[r][Q];
        W[r][P] = c * wp - s * wq;
        W[r][Q] = s * wp + c * wq;
        const double vp = V[r][P], vq = V[r][Q];
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
    return true;
}

UMEREG_POLAR_FN_INLINE void cross3(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// R = U diag(1, 1, det(U Vh)) Vh for A = U S Vh   (utils/loc_utils.py:326-329).
// With A = sum_i s_i u_i v_i^T this equals u0 v0^T + u1 v1^T + (u0 x u1)(v0 x v1)^T, which needs
// only the two dominant singular pairs and no sign bookkeeping.
UMEREG_POLAR_FN void polar_rotation(const double A[3][3], double R[3][3])
{
    // Scale by a power of two (exact) so that the largest entry is in [1, 2): the squares below neither overflow nor vanish and
    // the rank-1 threshold further down is relative to |A|.
    double amax = 0.0;
    bool nan = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            amax = fmax(amax, fabs(A[p][q]));   // (fmax skips a NaN: hence the flag)
            nan |= A[p][q] != A[p][q];
        }
    // A == 0: any rotation is optimal; LAPACK returns U = V = I -> R = I.  The same for an A with an infinite or NaN entry.
    if (!(amax > 0.0) || !(amax <= 1.7976931348623157e308) || nan) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q) R[p][q] = p == q ? 1.0 : 0.0;
        return;
    }
    const int sh = -ilogb(amax);
    double As[3][3], W[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) W[p][q] = As[p][q] = ldexp(A[p][q], sh);
    // cyclic sweeps until no pair needs a rotation (quadratic convergence: 3-5 sweeps)
    for (int sweep = 0; sweep < kPolarSweeps; ++sweep) {
        bool any = hestenes_rotate<0, 1>(W, V);
        any |= hestenes_rotate<0, 2>(W, V);
        any |= hestenes_rotate<1, 2>(W, V);
        if (!any) break;
    }
    // squared singular values = squared column norms; pick the two largest (branch-free selects keep everything in registers)
    const double l0 = W[0][0] * W[0][0] + W[1][0] * W[1][0] + W[2][0] * W[2][0];
    const double l1 = W[0][1] * W[0][1] + W[1][1] * W[1][1] + W[2][1] * W[2][1];
    const double l2 = W[0][2] * W[0][2] + W[1][2] * W[1][2] + W[2][2] * W[2][2];
    const int i_min = (l0 <= l1 && l0 <= l2) ? 0 : ((l1 <= l2) ? 1 : 2);
    double v0[3], v1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        v0[r] = i_min == 0 ? V[r][1] : V[r][0];
        v1[r] = i_min == 2 ? V[r][1] : V[r][2];
    }
    const double la = i_min == 0 ? l1 : l0, lb = i_min == 2 ? l1 : l2;
    if (lb > la) {
#pragma unroll
        for (int r = 0; r < 3; ++r) { const double tmp = v0[r]; v0[r] = v1[r]; v1[r] = tmp; }
    }
    double u0[3], u1[3];
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
    // rank 1: complete u1 with any unit vector orthogonal to u0.  Also when A v1 was a multiple of u0 (every column of A on one line:
    // s2 is rounding noise, and what the projection leaves is a rounding of that same line, which no re-orthogonalisation turns away)
    if (!(n1 > 1e-150) || !(n1 > 1e-8 * n1_raw)) {
        const int ax = (fabs(u0[0]) <= fabs(u0[1]) && fabs(u0[0]) <= fabs(u0[2])) ? 0
                       : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
        double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
        cross3(u0, e, u1);
        n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] /= n1;
    // once more: a u1 that was mostly cancellation (s2 at the rounding of s1) is not orthogonal to u0 after its normalisation
    const double d01b = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] -= d01b * u0[r];
    const double n1b = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] /= n1b;
    double u2[3], v2[3];
    cross3(u0, u1, u2);
    cross3(v0, v1, v2);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) R[p][q] = u0[p] * v0[q] + u1[p] * v1[q] + u2[p] * v2[q];
}

}  // namespace umereg
