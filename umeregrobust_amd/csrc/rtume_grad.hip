// rtume_grad.hip -- backward of a6, the closed-form SE(3) from a UME pair (rtume.hip: rtume_kernel without index arrays).
// C ABI: include/umereg_rtume_grad.h.
//
// The forward's shape: 32 lanes per hypothesis (lane = feature channel), two hypotheses per wavefront, group32_sum reductions,
// fp64 on the fp32 inputs, rounded once on output.  Nothing is saved by the forward: its 17 sums are formed again from G and H in
// the forward's own order, then the chain runs backwards -- T -> (R, b2) -> (A, wlc, wrc) -> (left, right) -> (g, h, mg, mh) --
// with 6 more sums (the columns of left and right against mg and mh).  The rotation's derivative is polar_grad.h.  A lane writes
// its own row of dG / dH as one float4: no atomics, no scratch, the same bits on every run.
#include "polar_grad.h"
#include "umereg_rtume_grad.h"

namespace umereg {

__global__ __launch_bounds__(256) void rtume_bwd_kernel(const float4* __restrict__ G_all, const float4* __restrict__ H_all,
                                                        const float* __restrict__ dT_all, int n, float4* __restrict__ dG,
                                                        float4* __restrict__ dH)
{
    const int row = threadIdx.x & 31;
    const int k = (int)blockIdx.x * 8 + (int)(threadIdx.x >> 5);  // (n / 8 workgroups: no product that could pass 2^31)
    if (k >= n) return;  // uniform per 32-lane group
    const float4 gv = G_all[(size_t)k * 32 + row];
    const float4 hv = H_all[(size_t)k * 32 + row];
    // ---- the forward again (rtume.hip, same order of operations) ----
    const double mg = gv.x, mh = hv.x;
    const double g[3] = {gv.y, gv.z, gv.w};
    const double h[3] = {hv.y, hv.z, hv.w};
    const double mg_square = group32_sum(mg * mg) + 1e-16;
    const double mg_mh = group32_sum(mg * mh);
    const double den_l = mg_square + 1e-16, den_r = mg_mh + 1e-16;
    double wlc[3], wrc[3], left[3], right[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        wlc[c] = group32_sum(g[c] * mg) / den_l;
        wrc[c] = group32_sum(h[c] * mg) / den_r;
        left[c] = g[c] - wlc[c] * mg;
        right[c] = h[c] - wrc[c] * mh;
    }
    double A[3][3];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) A[p][q] = group32_sum(left[p] * right[q]);
    // R as polar_rotation(A, R) forms it (the same operations: the forward's R)
    double U[3][3], V[3][3], s[3], R[3][3];
    const bool has_frames = polar_frames(A, U, V, s);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            R[p][q] = has_frames ? U[0][p] * V[0][q] + U[1][p] * V[1][q] + U[2][p] * V[2][q] : (p == q ? 1.0 : 0.0);
    // ---- T[:3,:3] = R^T, T[:3,3] = b2 = wrc - wlc @ R ----
    const float* dT = dT_all + (size_t)k * 16;
    double db2[3], gR[3][3], g_wlc[3], g_wrc[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) db2[q] = dT[q * 4 + 3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int q = 0; q < 3; ++q) gR[p][q] = (double)dT[q * 4 + p] - wlc[p] * db2[q];
        g_wlc[p] = -(R[p][0] * db2[0] + R[p][1] * db2[1] + R[p][2] * db2[2]);
        g_wrc[p] = db2[p];
    }
    // ---- R = polar_rotation(A); where the forward took R = I, no path through R ----
    double gA[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (has_frames) polar_rotation_grad(U, V, s, gR, UMEREG_RTUME_BWD_MIN_GAP, gA);
    // ---- A = left^T right ----
    double g_left[3], g_right[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g_left[c] = gA[c][0] * right[0] + gA[c][1] * right[1] + gA[c][2] * right[2];
        g_right[c] = gA[0][c] * left[0] + gA[1][c] * left[1] + gA[2][c] * left[2];
    }
    // ---- left = g - wlc mg, right = h - wrc mh ----
    double g_mg = 0.0, g_mh = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g_wlc[c] -= group32_sum(g_left[c] * mg);
        g_wrc[c] -= group32_sum(g_right[c] * mh);
        g_mg -= g_left[c] * wlc[c];
        g_mh -= g_right[c] * wrc[c];
    }
    // ---- wlc = gmg / (mg_square + 1e-16), wrc = hmg / (mg_mh + 1e-16) ----
    double g_gmg[3], g_hmg[3], g_sq = 0.0, g_mm = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g_gmg[c] = g_wlc[c] / den_l;
        g_hmg[c] = g_wrc[c] / den_r;
        g_sq -= g_gmg[c] * wlc[c];
        g_mm -= g_hmg[c] * wrc[c];
    }
    // ---- gmg = sum g mg, hmg = sum h mg, mg_square = sum mg^2 + 1e-16, mg_mh = sum mg mh ----
    double g_g[3], g_h[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g_g[c] = g_left[c] + g_gmg[c] * mg;
        g_h[c] = g_right[c] + g_hmg[c] * mg;
        g_mg += g_gmg[c] * g[c] + g_hmg[c] * h[c];
    }
    g_mg += 2.0 * g_sq * mg + g_mm * mh;
    g_mh += g_mm * mg;
    if (dG) dG[(size_t)k * 32 + row] = make_float4((float)g_mg, (float)g_g[0], (float)g_g[1], (float)g_g[2]);
    if (dH) dH[(size_t)k * 32 + row] = make_float4((float)g_mh, (float)g_h[0], (float)g_h[1], (float)g_h[2]);
}

}  // namespace umereg

using namespace umereg;

UMEREG_API int umereg_rtume_solve_bwd_f32(const float* G, const float* H, const float* dT, int n, float* dG, float* dH, void* stream)
{
    UMEREG_REQUIRE(G && H && dT, "rtume_solve_bwd: null pointer (G/H/dT)");
    UMEREG_REQUIRE(dG || dH, "rtume_solve_bwd: nothing to compute (dG and dH both null)");
    UMEREG_REQUIRE(n > 0, "rtume_solve_bwd: n must be positive (got %d)", n);
    UMEREG_REQUIRE(((uintptr_t)G & 15) == 0 && ((uintptr_t)H & 15) == 0 && ((uintptr_t)dG & 15) == 0 && ((uintptr_t)dH & 15) == 0 &&
                       ((uintptr_t)dT & 3) == 0,
                   "rtume_solve_bwd: misaligned pointer (G/H/dG/dH: 16 bytes)");
    if (int rc = check_device()) return rc;
    hipLaunchKernelGGL(rtume_bwd_kernel, dim3((unsigned)((n + 7LL) / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)G, (const float4*)H, dT, n, (float4*)dG, (float4*)dH);
    UMEREG_CHECK_LAUNCH("rtume_bwd_kernel");
    return UMEREG_OK;
}
